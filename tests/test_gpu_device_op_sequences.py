"""Chains of device ops and runs on one context (tests/device_op_sequences.py) on the MI355X: the committed seeds, and the cases
the generator aims at written out as step lists a reader can follow.  Every case runs through the same model and executor: each
step's expected output is the restatement (or the CPU oracle) applied to the model's expected input, nothing is read back between
steps, and at the end every buffer -- maps with their padding, counts between guards, lists with the canary behind them -- equals
the model byte for byte.

The pipelined contexts queue one hysteresis launch per run on 32-row tiles, and their first frames hold a weak chain across the
tiles: until finish_slot has continued such a run from the host its maps differ from the final ones
(test_the_neighbour_stays_in_flight reads that difference off the device), so a reader that was not ordered behind its writer
gives other points, lines and segments, every time."""
import math

import numpy as np
import pytest

import device_op_sequences as DS
from cudacam_amd import api

pytestmark = pytest.mark.gpu

PARTS = 7


@pytest.mark.parametrize("part", range(PARTS))
def test_seeds(oracle, part):
    for seed in DS.SEEDS[part::PARTS]:
        DS.run_seed(seed, oracle)


def _params(w=130, h=67, ch=1, mode="R", pipeline=True, per_channel=False, **more):
    P = dict(w=w, h=h, ch=ch, mode=mode, per_channel=per_channel, per_channel_ever=per_channel, pipeline=pipeline, low=10 if mode == "R" else 50,
             high=40 if mode == "R" else 150, hough_bound=0, pool_kinds=["chain0", "chain1", "natural", "wobble", "natural", "sparse"], pool_seeds=[1, 2, 3, 4, 5, 6])
    P.update(more)
    return P


def _run(f0, out, n=4, src="frames"):
    return dict(kind="run", src=src, f0=f0, n=n, out=out)


def _points(view, n, slot=0, cap=None, P=None):
    return dict(kind="points", view=view, n=n, slot=slot, cap=P["w"] * P["h"] if cap is None else cap)


def _lines(n, geo, lslot, lcap, P, pslot=0, threshold=6):
    return dict(kind="lines", pslot=pslot, pcap=P["w"] * P["h"], n=n, geo=geo, threshold=threshold, lslot=lslot, lcap=lcap)


def _segs(view, n, lslot, lcap, geo, sslot, scap=DS.SCAP_MAX, lgeo=None):
    return dict(kind="segs", view=view, n=n, lslot=lslot, lcap=lcap, lgeo=geo if lgeo is None else lgeo, geo=geo, min_length=3, max_gap=2, sslot=sslot, scap=scap)


def _circles(n, P, cslot=0, pslot=0, pcap=None, dp=1.0, min_dist=3.0, threshold=4, rmin=2, rmax=None, cc=4096, ccap=DS.CCAP_MAX):
    return dict(kind="circles", pslot=pslot, pcap=P["w"] * P["h"] if pcap is None else pcap, n=n, dp=dp, min_dist=min_dist, threshold=threshold, rmin=rmin,
                rmax=min(P["w"], P["h"]) // 2 if rmax is None else rmax, cc=cc, cslot=cslot, ccap=ccap)


def _deriv(n, f0=0, ksize=3):
    return dict(kind="deriv", f0=f0, n=n, ksize=ksize)


def _circle_counts(model, cslot, n):
    return model.words(f"circ{cslot}", model.L["counts_off"], n, np.uint32).tolist()


def _components(view, n, P, conn=8, cap=None, rows=True, cslot=0, over=None, lslot=0, loff=1, lpad=4, lgap=8):
    """A components step with a label plane of its own (padded rows, a gap between frames, 4 * loff bytes into its arena) -- or, with
    over=k, one frame of labels laid over output region k."""
    st = dict(kind="components", view=view, n=n, conn=conn, cap=P["w"] * P["h"] + 1 if cap is None else cap, rows=rows, cslot=cslot, dest="own", lslot=lslot, loff=loff, lpad=lpad, lgap=lgap)
    if over is not None:
        assert n == 1
        st.update(dest="over", lslot=over, loff=0, lpad=4 * (DS.layout(P)["op"] - P["w"]), lgap=0)
    return st


def _component_counts(model, cslot, n):
    return model.words(f"comp{cslot}", model.L["counts_off"], n, np.uint32).tolist()


RECT3 = (1, 1, 1)


def _morph(view, n, op=DS.MR.CLOSE, spans=RECT3, into=None, g0=0, mslot=0, moff=1, mpad=1, mgap=3, frames=None):
    """A morph step of a one-channel view (frames=f0: of 3-channel frames of the pool from f0 on) into arena mslot at an odd
    offset, pitch and frame stride -- or, with into=k, into frames g0 .. of output region k; into="sout" / "blur": of that buffer."""
    st = dict(kind="morph", src="view", view=view, f0=0, n=n, channels=1, op=op, spans=list(spans), dst="own", mslot=mslot, moff=moff, mpad=mpad, mgap=mgap, g0=0)
    if frames is not None:
        st.update(src="frames", view=None, f0=frames, channels=3)
    if into is not None:
        st.update(dst=into if isinstance(into, str) else "maps", mslot=0 if isinstance(into, str) else into, moff=0, mpad=0, mgap=0, g0=g0)
    return st


def _dist(view, n, P, target=api.DT_TO_NONZERO, dtype=api.DT_F32, over=None, dslot=0, near="none", swords=1, nleft=False, doff=1, dpad=4, dgap=8):
    """A dist step with the distance plane in arena dslot (padded rows, a gap between frames, 4 * doff bytes in) -- or, with over=k,
    one frame of it laid over output region k.  near: "none", "own" (the other arena, or with over=k arena dslot) or "side" (the
    second ROI of the distances' plane, 4 W + 4 * swords bytes to their right; nleft: to their left)."""
    own = near == "own"
    st = dict(kind="dist", view=view, n=n, target=target, dtype=dtype, dest="own", dslot=dslot, doff=doff, dpad=dpad, dgap=dgap, near=near, nslot=1 - dslot if own else 0,
              noff=2 if own else 0, npad=20 if own else 0, ngap=132 if own else 0, swords=swords if near == "side" else 0, nleft=nleft and near == "side")
    if over is not None:
        assert n == 1 and near != "side"
        st.update(dest="over", dslot=over, doff=0, dpad=4 * (DS.layout(P)["op"] - P["w"]), dgap=0, nslot=dslot if own else 0)
    return st


def _region(model, k, n):
    """The first n frames of output region k as the model holds them: (n, H, W) bytes."""
    L = model.L
    return model.get("maps", DS.out_start(L, k), L["op"], L["ofs"], n, model.w)


def _point_counts(model, slot, n):
    return model.words(f"pts{slot}", model.L["counts_off"], n, np.uint32).tolist()


def _blur(src, f0, dst, g0, n):
    return dict(kind="blur", src=src, f0=f0, dst=dst, g0=g0, n=n, ksize=5, sigma=1.2, border=0)


SYNC = dict(kind="sync")


@pytest.mark.parametrize("reader", ["points of the last frame", "segments of an ROI inside frame 2", "blur of frame 0", "blur into the buffer a staged run copies to"])
def test_partial_views_of_a_pending_output(oracle, reader):
    """Pipelined Mode R, four frames, runs into rotating outputs whose content needs the host continuation; then, with no
    synchronisation, a reader (or a writer) of PART of a pending output.  Each must complete the run first."""
    P = _params()
    staged = reader.startswith("blur into")
    steps = [_run(0, 0), _points(("whole", 0), 4, P=P), _lines(4, 0, 0, 64, P), SYNC,          # lines of the final maps, for the segment walk
             _run(0, 0), _run(1, "sout" if staged else 1)]                                  # ... and the same maps again, in flight
    kind = {"points": "frame", "segmen": "roi", "blur o": "blur_in", "blur i": "blur_out"}[reader[:6]]
    steps.append({"frame": _points(("frame", 0, 3), 1, slot=1, P=P), "roi": _segs(("roi", 0, 2, 3, 1, 1), 1, 0, 64, 0, 0),
                  "blur_in": _blur(0, 0, "blur", 0, 1), "blur_out": _blur("frames", 2, "sout", 1, 2)}[kind])
    with DS.Executor(P, oracle, reader) as e:
        for st in steps:
            e.queue(st)
            if st is SYNC:
                assert e.ctx.hysteresis_totals(reset=True)[:2] == (1, 1)   # the first run, complete: the count starts again
        assert e.model.counters[f"overlap_{kind}"] == 1, "the model sees no pending writer under this view"
        e.check()
        assert e.ctx.hysteresis_totals()[:2] == (2, 2), "the two runs in flight under the reader were not both continued from the host"
        if kind == "roi":
            assert e.model.counters["seg_lists_nonempty"] > 0


def test_the_neighbour_stays_in_flight(oracle):
    """Readers of a buffer that ends exactly where a pending output begins, and of one that begins exactly where it ends: right
    results, and the run is NOT completed for them.  hc_pipeline_slots_in_use does not say that (it is the size of the ring, 4
    before and after), and every getter of the last run's hysteresis completes the runs itself.  What shows an unfinished run is
    its output: once the device is idle it holds what the one queued launch left, which differs from the final map until
    finish_slot continues the run on the host -- at hc_sync here, not at the readers' calls."""
    import torch
    P = _params()
    L = DS.layout(P)
    with DS.Executor(P, oracle, "neighbours") as e:
        for st in (_run(0, 0), _run(1, 1)):
            e.queue(st)
        slots = e.ctx.pipeline_slots_in_use()
        e.queue(_points(("before", 0), 1, slot=0, P=P))
        e.queue(_points(("behind", 1, 4), 1, slot=1, P=P))
        assert e.model.counters["adjacent"] == 2 and not any(e.model.counters[f"overlap_{k}"] for k in DS.VIEW_KINDS)
        assert e.ctx.pipeline_slots_in_use() == slots == 4
        torch.cuda.synchronize()   # the device, not the context: no run is completed by this
        got, want = e.d["maps"].cpu().numpy(), e.model.buf["maps"]
        for k in (0, 1):
            a = DS.out_start(L, k)
            assert not np.array_equal(got[a:a + L["oreg"]], want[a:a + L["oreg"]]), f"output {k} already holds its final maps: its run was completed, or its content needs no continuation"
        e.check()
        assert e.continued_runs() == 2


@pytest.mark.parametrize("other", [1, 2], ids=["rho differs", "min_theta differs"])
def test_equal_numangle_other_tables(oracle, other):
    """Lines with geometry A, B, A, then segments with A, B, A, queued with no synchronisation: numangle is 12 for both, the tables
    are not.  Every result is that of its own geometry."""
    P = _params(w=250, h=66, mode="O", pipeline=False)
    steps = [_run(0, 0), _points(("whole", 0), 4, P=P)]
    steps += [_lines(4, g, s, 64, P) for g, s in ((0, 0), (other, 1), (0, 0))]
    steps += [_segs(("whole", 0), 4, s, 64, g, s) for g, s in ((0, 0), (other, 1), (0, 0))]
    assert DS.R.geometry(P["w"], P["h"], *DS.GEOS[0])[0] == DS.R.geometry(P["w"], P["h"], *DS.GEOS[other])[0] == 12
    model = DS.execute(P, steps, oracle, f"A, B = geometry {other}, A")
    c = model.counters
    assert c["hough_tables_equal_numangle"] == 2 and c["line_lists_nonempty"] == 12 and c["seg_lists_nonempty"] >= 8, c
    assert c["seg_tables_equal_numangle"] == 2
    assert not np.array_equal(model.buf["lines0"], model.buf["lines1"]), "A and B give the same lines for this input"


def _refused(call, entry, text="nframes out of range"):
    with pytest.raises(api.HipCannyError, match="error -1") as err:
        call()
    assert entry in str(err.value) and text in str(err.value), err.value


def test_three_channels_and_per_channel(oracle):
    """A 3-channel Mode R context with HC_OPT_PER_CHANNEL and max_batch 2: points, lines and segments take the 6 maps of a run and
    refuse 7; without the option they take 2 and refuse 3; switching the option between two chains leaves both right.  Blur,
    derivatives and automatic thresholds on the same context -- and circles, which take as many frames: of the gradient planes
    the entry reads the first W int16 of each interleaved row, in the frames behind the two that were written whatever is there."""
    P = _params(w=65, h=64, ch=3, pipeline=True, per_channel=True, max_batch=2)
    with DS.Executor(P, oracle, "per-channel") as e:
        def chain(n):
            for st in (_run(0, 0, n=2), _points(("whole", 0), n, P=P), _lines(n, 3, 0, 64, P), _segs(("whole", 0), n, 0, 64, 3, 0),
                       _blur("frames", 1, "blur", 0, 2), dict(kind="deriv", f0=2, n=2, ksize=7), _circles(n, P, threshold=8, cc=300), dict(kind="autothr", f0=0, n=2, rule=1, param=0.5)):
                e.queue(st)

        def at_the_limit_and_beyond(n):
            """Points, lines, segments and circles of n maps into the second slots with capacity 8 each: taken.  The same pointers,
            pitches and capacities with n + 1: refused for nframes, and nothing is written."""
            for st in (_points(("whole", 0), n, slot=1, cap=8), dict(kind="lines", pslot=1, pcap=8, n=n, geo=0, threshold=5, lslot=1, lcap=8), _segs(("whole", 0), n, 1, 8, 0, 1, scap=8)):
                e.queue(st)
            p, l, s = (e._counts(f"{b}1") for b in ("pts", "lines", "segs"))
            pl, ll, sl = (e._list(f"{b}1") for b in ("pts", "lines", "segs"))
            m, geo = e._view(("whole", 0)), DS.GEOS[0]
            _refused(lambda: e.ctx.edge_points_device(*m, n + 1, p, pl, 8), "hc_edge_points_device")
            _refused(lambda: e.ctx.hough_lines_device(pl, p, 8, n + 1, geo[0], geo[1], 5, geo[2], geo[3], l, ll, 8), "hc_hough_lines_device")
            _refused(lambda: e.ctx.hough_segments_device(*m, ll, l, 8, n + 1, *geo, 3, 2, s, sl, 8), "hc_hough_segments_device")
            e.queue(_circles(n, P, cslot=1, pslot=1, pcap=8, threshold=2, rmax=6, cc=300, ccap=8))
            (xo, pitch, fs), (yo, _, _) = e.model._planes(n)
            _refused(lambda: e.ctx.hough_circles_device(pl, p, 8, e.ptr["dxdy"] + xo, e.ptr["dxdy"] + yo, pitch, fs, n + 1, 1.0, 3.0, 2, 2, 6, 300, e._counts("circ1"), e._list("circ1"), 8),
                     "hc_hough_circles_device")
        chain(6)
        at_the_limit_and_beyond(6)
        e.check()
        assert e.model.counters["n_above_max_batch"] >= 6 and e.model.counters["seg_lists_nonempty"] > 0
        assert e.model.counters["circle_lists_nonempty"] > 0 and e.model.counters["circles_on_stale_frames"] == 2
        e.queue(dict(kind="option", option=api.OPT_PER_CHANNEL, value=0))
        chain(2)
        at_the_limit_and_beyond(2)
        e.check()
        e.queue(dict(kind="option", option=api.OPT_PER_CHANNEL, value=1))
        chain(6)
        e.check()
        assert e.continued_runs() > 0


def test_three_channels_mode_o(oracle):
    """The entries that had not met a 3-channel context: canny_device at every aperture, blur, derivatives chained with the gradient
    run, automatic thresholds installed as the table of a run -- then points, lines, segments and circles of what they wrote (the
    circles from a one-channel view of the interleaved Scharr planes, and in frame 3 of what no deriv step wrote)."""
    P = _params(w=61, h=33, ch=3, mode="O", pipeline=True)
    steps = [dict(kind="canny", f0=k, n=2, out=k % 3, low=DS.CANNY_THR[ap][0], high=DS.CANNY_THR[ap][1], aperture=ap, l2=int(ap == 5)) for k, ap in enumerate((3, 5, 7, -1))]
    steps += [_blur("frames", 0, "blur", 0, 4), dict(kind="autothr", f0=1, rule=0, param=0.33), dict(kind="thr_on"), _run(0, 1, src="blur"),
              dict(kind="deriv", f0=2, n=3, ksize=-1), dict(kind="rungrad", n=3, out=2), dict(kind="thr_off"),
              _points(("whole", 1), 4, P=P), _lines(4, 3, 0, DS.LCAP_MAX, P), _segs(("frame", 2, 2), 1, 0, DS.LCAP_MAX, 3, 0), _circles(4, P),
              _points(("whole", 0), 2, slot=1, cap=5, P=P)]
    model = DS.execute(P, steps, oracle, "3 channels, mode O")
    assert model.counters["circle_lists_nonempty"] > 0 and model.counters["circles_on_stale_frames"] == 1


def test_growth_across_entries(oracle):
    """One context, six calls queued with no synchronisation, each entry's second call needing more scratch than its first: points
    of one frame then four, lines at PI / 12 then PI / 180 (tables and accumulators grow), segments of 4 lines then 400 per frame."""
    P = _params(w=250, h=66, mode="R", pipeline=True)
    steps = [_run(0, 0), _points(("frame", 0, 1), 1, slot=1, P=P), _points(("whole", 0), 4, slot=0, P=P), _lines(1, 0, 0, 4, P), _lines(4, 3, 1, DS.LCAP_MAX, P),
             _segs(("whole", 0), 1, 0, 4, 0, 0), _segs(("whole", 0), 4, 1, DS.LCAP_MAX, 3, 1)]
    model = DS.execute(P, steps, oracle, "growth")
    assert model.counters["scratch_growths"] == 2 and model.counters["seg_lists_nonempty"] >= 4 and model.counters["lists_cut"] > 0, model.counters


# ---- circles in company: hc_hough_circles_device chained behind the entries that write its inputs, between the Hough-line calls it
# shares a scratch bound with, and on contexts with runs in flight.  tests/test_gpu_hough_circles.py has the kernels, call by call.
def test_lines_and_circles_alternate_under_one_bound(oracle):
    """Five calls queued with no synchronisation under the one bound of both scratches (two frames of the 180-angle line geometry):
    lines of that geometry take two passes of two frames, circles with 4096 centres two passes of three and one, lines of twelve
    angles and circles with 16 centres one pass -- each with its own scratch, cut by its own plan."""
    w, h = 61, 33
    P = _params(w=w, h=h, mode="O", pipeline=False, hough_bound=2 * DS.hough_need(w, h, DS.GEO_BIG, 1, 0)[2])
    first, second = _circles(4, P, cslot=0, dp=1.0, cc=4096), _circles(4, P, cslot=1, dp=2.0, cc=16)
    steps = [_run(0, 0), _points(("whole", 0), 4, P=P), _deriv(4), _lines(4, 3, 0, DS.LCAP_MAX, P), first, _lines(4, 0, 1, 64, P), second, _lines(4, 3, 0, DS.LCAP_MAX, P)]
    assert DS.hough_need(w, h, DS.GEO_BIG, 4, P["hough_bound"])[1] == 2 and DS.hough_need(w, h, DS.GEO_A, 4, P["hough_bound"])[1] == 1
    assert [DS.circle_need(w, h, st["dp"], st["cc"], 4, P["hough_bound"])[1] for st in (first, second)] == [2, 1]
    model = DS.execute(P, steps, oracle, "lines and circles under one bound")
    c = model.counters
    assert c["hough_passes_above_one"] == 2 and c["circle_passes_above_one"] == 1 and c["circles_between_lines"] == 2, c
    assert min(_circle_counts(model, 0, 4)) > 0 and min(_circle_counts(model, 1, 4)) > 0 and c["line_lists_nonempty"] == 12, c


def test_the_real_chain_pipelined(oracle):
    """cv::Canny, its derivatives, the edge points and the circles of four frames, queued with no synchronisation on a pipelined
    context: the point reader completes the run (its content needs the host continuation), the circles follow on the stream.
    Then circles of the same lists again while runs into two OTHER outputs are in flight: no run writes a point list or a
    gradient plane, so the entry completes none of them -- read off the device as test_the_neighbour_stays_in_flight reads it."""
    import torch
    P = _params(w=130, h=67, mode="O", pipeline=True)
    L = DS.layout(P)
    with DS.Executor(P, oracle, "the real chain") as e:
        for st in (dict(kind="canny", f0=0, n=4, out=0, low=DS.CANNY_THR[3][0], high=DS.CANNY_THR[3][1], aperture=3, l2=0), _deriv(4), _points(("whole", 0), 4, P=P),
                   _circles(4, P, cslot=0)):
            e.queue(st)
        assert e.model.counters["overlap_whole"] == 1 and not e.model.pending
        e.check()
        assert min(_circle_counts(e.model, 0, 4)) > 0 and e.model.counters["circles_on_stale_frames"] == 0
        before = e.continued_runs()
        assert before > 0
        for st in (_run(0, 1), _run(0, 2, n=2)):
            e.queue(st)
        e.queue(_circles(4, P, cslot=1, dp=2.0))
        assert len(e.model.pending) == 2 and e.model.counters["overlap_whole"] == 1
        torch.cuda.synchronize()   # the device, not the context: no run is completed by this
        got, want = e.d["maps"].cpu().numpy(), e.model.buf["maps"]
        for k, n in ((1, 4), (2, 2)):
            a = DS.out_start(L, k)
            assert not np.array_equal(got[a:a + n * L["ofs"]], want[a:a + n * L["ofs"]]), f"output {k} already holds its final maps: the circles call completed its run, or its content needs no continuation"
        e.check()
        assert min(_circle_counts(e.model, 1, 4)) > 0 and e.continued_runs() == before + 2


def test_circles_of_planes_nobody_wrote_and_of_stale_frames(oracle):
    """The gradient planes are the caller's bytes: before any derivative call they hold what the allocation held (here int16 -1,
    -1 everywhere: every ray a diagonal), behind the frames of the last call what an earlier one left.  Circles of exactly that."""
    P = _params(w=65, h=64, mode="R", pipeline=True)
    steps = [_run(0, 0), _points(("whole", 0), 4, P=P), _circles(4, P, cslot=0), _deriv(2), _circles(4, P, cslot=1), _deriv(4, f0=1, ksize=7), _deriv(1, f0=2, ksize=3),
             _circles(4, P, cslot=0, dp=1.5)]
    model = DS.execute(P, steps, oracle, "unwritten and stale planes")
    c = model.counters
    assert c["circles_on_unwritten_planes"] == 1 and c["circles_on_stale_frames"] == 2 and c["circle_lists_nonempty"] >= 8, c


def test_circle_scratch_grows_while_a_call_is_queued(oracle):
    """One frame with 16 centres at dp 2, then four frames with 4096 at dp 1 (the scratch is allocated again, behind a
    synchronisation of the stream the first call is queued on), then the first call again into the other slot: in the larger
    scratch its sections lie elsewhere, its circles are the same."""
    P = _params(w=250, h=66, mode="R", pipeline=False)
    small = dict(dp=2.0, cc=16, threshold=3)
    steps = [_run(0, 0), _points(("whole", 0), 4, P=P), _deriv(4), _circles(1, P, cslot=0, **small), _circles(4, P, cslot=1, dp=1.0, cc=4096, threshold=3), _circles(1, P, cslot=1, **small)]
    model = DS.execute(P, steps, oracle, "circle scratch growth")
    assert model.counters["circle_scratch_growths"] == 1, model.counters
    (k0,), (k1,) = _circle_counts(model, 0, 1), _circle_counts(model, 1, 1)
    assert k0 == k1 > 0 and np.array_equal(model.words("circ0", model.L["list_off"], 4 * k0, np.int32), model.words("circ1", model.L["list_off"], 4 * k0, np.int32))


def test_circles_of_cut_inputs_and_into_cut_outputs(oracle):
    """Point lists cut by their capacity (the stored counts stay above it), centres cut by centre_capacity, circles cut by
    circle_capacity 8, and circle_capacity 0 with a pointer: the counts alone, the lists of the call before untouched."""
    P = _params(w=130, h=67, mode="R", pipeline=True)
    steps = [_run(0, 0), _deriv(4), _points(("whole", 0), 4, slot=1, cap=5, P=P), _circles(4, P, cslot=0, pslot=1, pcap=5, threshold=1, min_dist=0.0, rmin=1, rmax=6),
             _points(("whole", 0), 4, slot=0, P=P), _circles(4, P, cslot=1, cc=16, threshold=2), _circles(4, P, cslot=0, ccap=8, threshold=2), _circles(4, P, cslot=1, ccap=0, threshold=2, dp=1.5)]
    with DS.Executor(P, oracle, "cut inputs and outputs") as e:
        seen = []
        for st in steps:
            e.queue(st)
            seen.append(dict(e.model.counters))
        e.check()
    assert seen[3]["circles_from_cut_points"] == 4 and seen[3]["lists_cut"] == 4, seen[3]
    assert seen[5]["circles_centres_cut"] > 0 and seen[5]["circle_lists_nonempty"] > seen[4]["circle_lists_nonempty"], seen[5]
    assert seen[6]["circle_lists_cut"] > seen[5]["circle_lists_cut"] and seen[7]["circle_lists_cut"] == seen[6]["circle_lists_cut"], seen[7]
    assert seen[7]["circle_lists_nonempty"] > seen[6]["circle_lists_nonempty"], seen[7]


def test_circles_across_a_stream_switch(oracle):
    """Circles on the context's own stream, on a caller's stream and on its own again, each switch behind a synchronisation as
    include/hipcanny.h asks of calls that share scratch; the second geometry needs a larger scratch than the first."""
    P = _params(w=61, h=33, mode="R", pipeline=True)
    steps = [_run(0, 0), _points(("whole", 0), 4, P=P), _deriv(4), _circles(4, P, cslot=0, dp=2.0, cc=16), SYNC, dict(kind="stream", to="side"),
             _circles(4, P, cslot=1, dp=1.0, cc=4096, rmin=3, rmax=66), SYNC, dict(kind="stream", to="own"), _circles(2, P, cslot=0, dp=1.5, cc=300)]
    model = DS.execute(P, steps, oracle, "circles across a stream switch")
    assert model.counters["circle_lists_nonempty"] >= 6 and model.counters["circle_scratch_growths"] == 1, model.counters


# ---- components in company: hc_connected_components_device reads edge maps AND writes a plane the caller chooses, so it completes
# the runs in flight under either; its table of per-chunk counts is the third scratch under the context's one bound.
# tests/test_gpu_connected_components.py has the kernels, call by call.
def test_labels_over_a_pending_output(oracle):
    """Two pipelined runs into outputs 0 and 1 whose content needs the host continuation; then, with no synchronisation, the
    components of frame 1 of output 1 with the label plane laid OVER output 0, then the points of output 0 -- of the label bytes.
    The entry must continue run 0 before its kernels write there: continued later (by the points call, or at the sync), the run
    rewrites its whole maps over the labels."""
    P = _params()
    with DS.Executor(P, oracle, "labels over a pending output") as e:
        for st in (_run(0, 0), _run(1, 1), _components(("frame", 1, 1), 1, P, over=0), _points(("whole", 0), 4, P=P)):
            e.queue(st)
        c = e.model.counters
        assert c["components_labels_over_pending"] == 1 and c["components_overlap_map"] == 1 and c["overlap_frame"] == 1 and c["overlap_whole"] == 0 and not e.model.pending, c
        e.check()
        assert e.continued_runs() == 2 and _component_counts(e.model, 0, 1)[0] > 9
        (n0,) = e.model.words("pts0", e.model.L["counts_off"], 1, np.uint32).tolist()
        assert n0 > P["w"]   # the points of frame 0 are the non-zero bytes of the labels' first rows


def test_components_behind_runs_left_in_flight(oracle):
    """Three pipelined runs into the three outputs, then the components of the LAST frame of output 1 into a plane of their own:
    run 1 is completed, its neighbours are not -- read off the device as test_the_neighbour_stays_in_flight reads it."""
    import torch
    P = _params()
    L = DS.layout(P)
    with DS.Executor(P, oracle, "components behind runs in flight") as e:
        for st in (_run(0, 0), _run(0, 1), _run(0, 2), _components(("frame", 1, 3), 1, P, conn=4)):
            e.queue(st)
        c = e.model.counters
        assert c["overlap_frame"] == 1 and c["components_overlap_map"] == 1 and c["components_labels_over_pending"] == 0 and len(e.model.pending) == 2, c
        torch.cuda.synchronize()   # the device, not the context: no run is completed by this
        got, want = e.d["maps"].cpu().numpy(), e.model.buf["maps"]
        for k in (0, 2):
            a = DS.out_start(L, k)
            assert not np.array_equal(got[a:a + L["oreg"]], want[a:a + L["oreg"]]), f"output {k} already holds its final maps: the components call completed its run, or its content needs no continuation"
        a = DS.out_start(L, 1)
        assert np.array_equal(got[a:a + L["oreg"]], want[a:a + L["oreg"]]), "output 1 does not hold its final maps behind the call that read it"
        e.check()
        assert e.continued_runs() == 3 and _component_counts(e.model, 0, 1)[0] > 2


def test_components_in_passes_under_a_bound(oracle):
    """67 rows are 9 chunks of 8: 36 bytes of table per frame.  Under a bound of 39 bytes four frames take four passes, under 75
    two; then, with the default bound again, lines, circles and components follow one another with no synchronisation -- the
    accumulators, the circle scratch and the table are three buffers under one bound -- and the components are the same."""
    P = _params(pipeline=False)
    per = DS.ccl_need(P["h"], 4, 0)[2]
    assert per == 36 and [DS.ccl_need(P["h"], 4, b)[1] for b in (per + 3, 2 * per + 3, 0)] == [4, 2, 1]
    bound = lambda v: dict(kind="option", option=api.OPT_TEST_HOUGH_SCRATCH, value=v)
    steps = [_run(0, 0), bound(per + 3), _components(("whole", 0), 4, P, cslot=0, lslot=0), bound(2 * per + 3), _components(("whole", 0), 4, P, conn=4, cap=5, cslot=0, lslot=0),
             bound(0), _points(("whole", 0), 4, P=P), _deriv(4), _lines(4, 3, 0, DS.LCAP_MAX, P), _circles(4, P, cc=300), _components(("whole", 0), 4, P, cslot=1, lslot=1, loff=0, lpad=0),
             _lines(4, 0, 1, 64, P)]
    with DS.Executor(P, oracle, "components in passes") as e:
        for i, st in enumerate(steps):
            e.queue(st)
            if i == 2:   # what four passes left, before the second call writes into the same slots
                e.check()
                first = {k: e.model.buf[k].copy() for k in ("comp0", "lab0")}
        e.check()
        c, L = e.model.counters, e.model.L
        assert c["ccl_passes_above_one"] == 2 and c["components_rows_cut"] == 4 and c["circle_lists_nonempty"] == 4 and c["line_lists_nonempty"] == 8, c
        assert np.array_equal(first["comp0"], e.model.buf["comp1"]), "one pass gives other rows than four"
        lab = lambda b, st: b[e.model._index(*DS.label_view(L, st)[1:], 4, P["h"], 4 * P["w"])]
        assert np.array_equal(lab(first["lab0"], steps[2]), lab(e.model.buf["lab1"], steps[10])), "one pass gives other labels than four"
        assert min(_component_counts(e.model, 1, 4)) > 1 and max(_component_counts(e.model, 1, 4)) > 9


def test_the_component_table_grows_while_a_call_is_queued(oracle):
    """One frame (the third of the output, a natural one), then four (the table is allocated again, behind a synchronisation of the stream the first call is queued on),
    then a lines call, then the first call again into the other slot: the same rows."""
    P = _params(w=250, h=66, pipeline=False)
    steps = [_run(0, 0), _points(("whole", 0), 4, P=P), _components(("frame", 0, 2), 1, P, cslot=0, lslot=0), _components(("whole", 0), 4, P, conn=4, cslot=1, lslot=1),
             _lines(4, 3, 0, DS.LCAP_MAX, P), _components(("frame", 0, 2), 1, P, cslot=1, lslot=1)]
    with DS.Executor(P, oracle, "component table growth") as e:
        for st in steps[:-1]:
            e.queue(st)
        four = _component_counts(e.model, 1, 4)
        e.queue(steps[-1])
        e.check()
        m = e.model
        assert m.counters["ccl_scratch_growths"] == 1 and m.counters["line_lists_nonempty"] == 4, m.counters
        (k0,), now = _component_counts(m, 0, 1), _component_counts(m, 1, 4)
        assert now[0] == k0 > 9 and now[1:] == four[1:] and min(four) > 2
        assert np.array_equal(m.words("comp0", m.L["stats_off"], 5 * k0, np.int32), m.words("comp1", m.L["stats_off"], 5 * k0, np.int32))


def test_components_per_channel(oracle):
    """A 3-channel Mode R context with HC_OPT_PER_CHANNEL and max_batch 2: the components of the 6 maps of a run, 7 refused; with
    the option off 2 are taken and 3 refused, and nothing is written by a refused call."""
    P = _params(w=65, h=64, ch=3, pipeline=True, per_channel=True, max_batch=2)
    with DS.Executor(P, oracle, "components per channel") as e:
        def at_the_limit_and_beyond(n):
            e.queue(_components(("whole", 0), n, P, conn=4, cap=5, cslot=1, lslot=1))
            (lname, loff, lpitch, lfs), o = DS.label_view(e.L, e.steps[-1]), "comp1"
            _refused(lambda: e.ctx.connected_components_device(*e._view(("whole", 0)), n + 1, 8, e.ptr[lname] + loff, lpitch, lfs, e._counts(o), e.ptr[o] + e.L["stats_off"],
                                                               e.ptr[o] + e.L["cent_off"], 5), "hc_connected_components_device")
        e.queue(_run(0, 0, n=2))
        e.queue(_components(("whole", 0), 6, P, conn=4, cslot=0, lslot=0))
        at_the_limit_and_beyond(6)
        e.check()
        c = e.model.counters
        assert c["components_n_above_max_batch"] == 2 and c["components_overlap_map"] == 1 and c["components_rows_cut"] == 6 and min(_component_counts(e.model, 0, 6)) > 5, c
        e.queue(dict(kind="option", option=api.OPT_PER_CHANNEL, value=0))
        e.queue(_run(1, 1, n=2))
        e.queue(_components(("whole", 1), 2, P, conn=4, cslot=0, lslot=0))
        at_the_limit_and_beyond(2)
        e.check()
        assert e.continued_runs() > 0


def test_components_across_a_stream_switch(oracle):
    """Components on the context's own stream, on a caller's stream and on its own again, each switch behind a synchronisation as
    include/hipcanny.h asks of calls that share scratch; the second call needs a larger table than the first, and lays its labels
    over an output."""
    P = _params(w=61, h=33, pipeline=True)
    steps = [_run(0, 0), _run(1, 1), _components(("whole", 0), 2, P, cslot=0), SYNC, dict(kind="stream", to="side"), _components(("whole", 1), 4, P, conn=4, cslot=1, lslot=1), SYNC,
             dict(kind="stream", to="own"), _components(("frame", 0, 2), 1, P, cap=3, over=2), _points(("whole", 2), 1, P=P)]
    model = DS.execute(P, steps, oracle, "components across a stream switch")
    c = model.counters
    assert c["ccl_scratch_growths"] == 1 and c["components_overlap_map"] == 1 and c["components_rows_cut"] == 1 and min(_component_counts(model, 1, 4)) > 2, c


# ---- morphology and distances in company: hc_morphology_device and hc_distance_transform_device read edge maps AND write views the
# caller chooses, so each completes the runs in flight under all of its views; OPEN / CLOSE keep their intermediate frames in the
# fourth scratch under the context's one bound; the distance transform keeps its intermediate values in the caller's own plane.
# tests/test_gpu_morphology.py and tests/test_gpu_distance_transform.py have the kernels, call by call.
def test_morphology_and_distances_over_pending_outputs(oracle):
    """Three pipelined runs into the three outputs whose content needs the host continuation; then, with no synchronisation, CLOSE
    of output 0 INTO output 1, the distances of frame 1 of output 1 with the plane laid OVER output 2 (the nearest plane in an
    arena), and the points of outputs 1 and 2.  Each entry must continue the run under the view it writes before its kernels write
    there: continued later (by the points calls, or at the sync), the run rewrites its whole maps over the result."""
    P = _params()
    with DS.Executor(P, oracle, "morphology and distances over pending outputs") as e:
        for st in (_run(0, 0), _run(0, 1), _run(0, 2)):
            e.queue(st)
        runs = [_region(e.model, k, 4).copy() for k in range(3)]
        e.queue(_morph(("whole", 0), 4, into=1))
        c = e.model.counters
        assert c["morph_overlap_in"] == 1 and c["morph_out_over_pending"] == 1 and len(e.model.pending) == 1, c
        e.queue(_dist(("frame", 1, 1), 1, P, over=2, near="own"))
        assert c["dist_plane_over_pending"] == 1 and c["dist_overlap_map"] == 0 and c["dist_of_morph_output"] == 1 and not e.model.pending, c
        for st in (_points(("whole", 1), 4, slot=0, P=P), _points(("whole", 2), 4, slot=1, P=P)):
            e.queue(st)
        assert c["morph_read_by_a_later_step"] == 2 and c["dist_plane_read_as_map"] == 1 and c["overlap_whole"] == 1, c   # (the one: the CLOSE, of output 0)
        e.check()
        assert e.continued_runs() == 3
        closed = DS.MR.morph(runs[0], DS.MR.CLOSE, list(RECT3))
        plane = DS.DR.root_f32(DS.DR.brute_force(closed[1])[0])   # one frame of float32 over the region's four frames of bytes
        a, L = DS.out_start(e.L, 2), e.L
        over = np.full(4 * L["ofs"], 255, np.uint8).reshape(4, P["h"], L["op"])   # the region as run 2 left it inside its padding ...
        over[:, :, :P["w"]] = runs[2]
        over.reshape(P["h"], -1)[:, :4 * P["w"]] = plane.view(np.uint8)          # ... and the plane's rows, 4 W bytes at four times the pitch
        assert np.array_equal(over.reshape(-1), e.model.buf["maps"][a:a + 4 * L["ofs"]])
        want = [[int(np.count_nonzero(m)) for m in closed], [int(np.count_nonzero(f[:, :P["w"]])) for f in over]]
        assert [_point_counts(e.model, 0, 4), _point_counts(e.model, 1, 4)] == want, want
        for k, counts in ((1, want[0]), (2, want[1])):   # a run continued after the entry wrote would leave its own maps, with other counts
            assert [int(np.count_nonzero(m)) for m in runs[k]] != counts, k


def test_morphology_and_distances_leave_other_runs_in_flight(oracle):
    """Three pipelined runs into the three outputs, then the GRADIENT of the LAST frame of output 1 into an arena and the distances
    of an ROI of output 1: run 1 is completed, its neighbours are not -- read off the device as test_the_neighbour_stays_in_flight
    reads it."""
    import torch
    P = _params()
    L = DS.layout(P)
    with DS.Executor(P, oracle, "morphology and distances behind runs in flight") as e:
        for st in (_run(0, 0), _run(0, 1), _run(0, 2), _morph(("frame", 1, 3), 1, op=DS.MR.GRADIENT, spans=DS.MORPH_ASYM[1]), _dist(("roi", 1, 0, 3, 1, 1), 1, P, near="side")):
            e.queue(st)
        c = e.model.counters
        assert c["morph_overlap_in"] == 1 and c["overlap_frame"] == 1 and c["morph_out_over_pending"] == 0 and c["dist_overlap_map"] == 0 and c["dist_plane_over_pending"] == 0, c
        assert len(e.model.pending) == 2
        torch.cuda.synchronize()   # the device, not the context: no run is completed by this
        got, want = e.d["maps"].cpu().numpy(), e.model.buf["maps"]
        for k in (0, 2):
            a = DS.out_start(L, k)
            assert not np.array_equal(got[a:a + L["oreg"]], want[a:a + L["oreg"]]), f"output {k} already holds its final maps: one of the calls completed its run, or its content needs no continuation"
        a = DS.out_start(L, 1)
        assert np.array_equal(got[a:a + L["oreg"]], want[a:a + L["oreg"]]), "output 1 does not hold its final maps behind the calls that read it"
        e.check()
        assert e.continued_runs() == 3 and c["morph_output_differs"] == 1 and c["dist_maps_mixed"] == 1, c


def test_morphology_in_passes_under_a_bound(oracle):
    """An intermediate frame of 130 x 67 is 132 x 67 = 8844 bytes.  OPEN and CLOSE of four maps under bounds of one, two and four
    such frames and a few bytes (four, two and one pass) give the same bytes; then, with the default bound again, lines, circles,
    components, CLOSE and lines follow one another with no synchronisation -- four buffers under one bound.  A bound one byte below
    a frame is refused, and the refused call writes nothing."""
    P = _params(pipeline=False)
    per = DS.morph_need(P["w"], P["h"], 1, DS.MR.OPEN, 4, 0)[2]
    assert per == 8844 and [DS.morph_need(P["w"], P["h"], 1, DS.MR.CLOSE, 4, b)[1] for b in (per + 3, 2 * per + 3, 4 * per + 3, 0, per - 1)] == [4, 2, 1, 1, 0]
    bound = lambda v: dict(kind="option", option=api.OPT_TEST_HOUGH_SCRATCH, value=v)
    open4, close4 = _morph(("whole", 0), 4, op=DS.MR.OPEN, spans=DS.MORPH_ASYM[0], mslot=0), _morph(("whole", 0), 4, op=DS.MR.CLOSE, spans=DS.MR.structuring_spans(DS.MR.ELLIPSE, 5), mslot=1)
    with DS.Executor(P, oracle, "morphology in passes") as e:
        e.queue(_run(0, 0))
        seen = []
        for b in (per + 3, 2 * per + 3, 4 * per + 3):
            for st in (bound(b), open4, close4):
                e.queue(st)
            e.check()
            seen.append({k: e.d[k].cpu().numpy() for k in ("mor0", "mor1")})   # (equal to the model's: the check has passed)
            for k in ("mor0", "mor1"):   # ... and the next bound starts from the arena's fill
                e.model.buf[k][:] = 255
                e.d[k].fill_(255)
            e.torch.cuda.synchronize()
        assert e.model.counters["morph_passes_above_one"] == 4 and e.model.counters["morph_output_differs"] == 6, e.model.counters
        assert all(np.array_equal(seen[0][k], s[k]) for s in seen[1:] for k in ("mor0", "mor1")), "the passes give other bytes than one pass"
        assert not np.array_equal(seen[0]["mor0"], seen[0]["mor1"]) and (seen[0]["mor0"] != 255).any()
        for st in (bound(0), _points(("whole", 0), 4, P=P), _deriv(4), _lines(4, 3, 0, DS.LCAP_MAX, P), _circles(4, P, cc=300), _components(("whole", 0), 4, P), close4, _lines(4, 0, 1, 64, P)):
            e.queue(st)
        e.check()
        assert np.array_equal(e.model.buf["mor1"], seen[0]["mor1"]) and e.model.counters["circle_lists_nonempty"] == 4 and e.model.counters["line_lists_nonempty"] == 8, e.model.counters
        e.queue(bound(per - 1))
        (a, aoff, ap, afs), (b, boff, bp, bfs) = DS.morph_views(e.L, open4)
        for op in (DS.MR.OPEN, DS.MR.CLOSE):
            _refused(lambda: e.ctx.morphology_device(e.ptr[a] + aoff, ap, afs, e.ptr[b] + boff, bp, bfs, 1, 1, op, 3, list(RECT3)), "hc_morphology_device", "scratch bound")
        e.queue(_morph(("whole", 0), 4, op=DS.MR.GRADIENT, mslot=0))   # (no intermediate frames: any bound)
        e.check()


def test_the_morphology_scratch_grows_while_a_call_is_queued(oracle):
    """CLOSE of one frame (the third of the output, a natural one), then of four (the scratch is allocated again, behind a
    synchronisation of the stream the first call is queued on), then a lines call, then the first call again into the other arena:
    the same bytes."""
    P = _params(w=250, h=66, pipeline=False)
    one = lambda mslot: _morph(("frame", 0, 2), 1, spans=DS.MR.structuring_spans(DS.MR.CROSS, 5), mslot=mslot)
    steps = [_run(0, 0), _points(("whole", 0), 4, P=P), one(0), _morph(("whole", 0), 4, spans=DS.MR.structuring_spans(DS.MR.RECT, 7), mslot=1), _lines(4, 3, 0, DS.LCAP_MAX, P), one(1)]
    model = DS.execute(P, steps, oracle, "morphology scratch growth")
    assert model.counters["morph_scratch_growths"] == 1 and model.counters["line_lists_nonempty"] == 4 and model.counters["morph_output_differs"] == 3, model.counters
    first, again = (model.get(*DS.morph_views(model.L, one(k))[1], 1, P["w"]) for k in (0, 1))
    assert np.array_equal(first, again) and first.any() and not np.array_equal(first, _region(model, 0, 3)[2:])


def test_morphology_and_distances_per_channel(oracle):
    """A 3-channel Mode R context with HC_OPT_PER_CHANNEL and max_batch 2: both entries take the 6 maps of a run and refuse 7, the
    morphology takes 2 3-channel frames and refuses 3; with the option off 2 maps are taken and 3 refused.  Nothing is written by a
    refused call."""
    P = _params(w=65, h=64, ch=3, pipeline=True, per_channel=True, max_batch=2)
    with DS.Executor(P, oracle, "morphology and distances per channel") as e:
        def at_the_limit_and_beyond(n, k):
            taken = (_morph(("whole", k), n, op=DS.MR.OPEN, spans=DS.MORPH_ASYM[2], mslot=0), _dist(("whole", k), n, P, dtype=api.DT_SQUARED_I32, near="own"))
            for st in taken:
                e.queue(st)
            (a, aoff, ap, afs), (b, boff, bp, bfs) = DS.morph_views(e.L, taken[0])
            _refused(lambda: e.ctx.morphology_device(e.ptr[a] + aoff, ap, afs, e.ptr[b] + boff, bp, bfs, n + 1, 1, DS.MR.DILATE, 3, list(RECT3)), "hc_morphology_device")
            (dn, doff, dp, dfs), (nn, noff, npitch, nfs) = DS.dist_views(e.L, taken[1])
            _refused(lambda: e.ctx.distance_transform_device(*e._view(("whole", k)), n + 1, 0, 0, e.ptr[dn] + doff, dp, dfs, e.ptr[nn] + noff, npitch, nfs), "hc_distance_transform_device")
            three = _morph(None, 2, op=DS.MR.GRADIENT, spans=DS.MR.structuring_spans(DS.MR.ELLIPSE, 7), mslot=1, frames=1)
            e.queue(three)
            (a, aoff, ap, afs), (b, boff, bp, bfs) = DS.morph_views(e.L, three)
            _refused(lambda: e.ctx.morphology_device(e.ptr[a] + aoff, ap, afs, e.ptr[b] + boff, bp, bfs, 3, 3, DS.MR.DILATE, 3, list(RECT3)), "hc_morphology_device")
        e.queue(_run(0, 0, n=2))
        at_the_limit_and_beyond(6, 0)
        e.check()
        c = e.model.counters
        assert c["morph_n_above_max_batch"] == 1 and c["dist_n_above_max_batch"] == 1 and c["morph_three_channel"] == 1 and c["morph_overlap_in"] == 1 and c["dist_maps_mixed"] == 1, c
        e.queue(dict(kind="option", option=api.OPT_PER_CHANNEL, value=0))
        e.queue(_run(1, 1, n=2))
        at_the_limit_and_beyond(2, 1)
        e.check()
        assert c["morph_overlap_in"] == 2 and c["morph_three_channel"] == 2 and e.continued_runs() > 0, c


def test_morphology_and_distances_across_a_stream_switch(oracle):
    """Both entries on the context's own stream, on a caller's stream and on its own again, each switch behind a synchronisation as
    include/hipcanny.h asks of calls that share scratch; the second CLOSE needs a larger scratch than the first, and the distances
    on the caller's stream lay their plane over an output, which the calls behind the second switch read as a map."""
    P = _params(w=61, h=33, pipeline=True)
    steps = [_run(0, 0), _run(1, 1), _morph(("whole", 0), 1, mslot=0), _dist(("whole", 0), 2, P, near="side", nleft=True), SYNC, dict(kind="stream", to="side"),
             _morph(("whole", 1), 4, spans=DS.MORPH_ASYM[1], mslot=1), _dist(("frame", 0, 2), 1, P, target=api.DT_TO_ZERO, dtype=api.DT_SQUARED_I32, over=2, near="own"), SYNC,
             dict(kind="stream", to="own"), _morph(("whole", 2), 2, op=DS.MR.OPEN, mslot=0), _points(("whole", 2), 1, P=P), _dist(("whole", 2), 1, P, dslot=1)]
    model = DS.execute(P, steps, oracle, "morphology and distances across a stream switch")
    c = model.counters
    assert c["morph_scratch_growths"] == 1 and c["morph_overlap_in"] == 1 and c["dist_plane_read_as_map"] == 3 and c["dist_side_by_side"] == 1 and c["dist_maps_mixed"] == 3, c


def test_the_real_chain_closed_labelled_and_measured(oracle):
    """cv::Canny, cv::morphologyEx(MORPH_CLOSE) with a 3 x 3 rectangle into another region, the components of the closed maps, the
    distances to the nearest edge as float32 with the nearest pixel beside them in one plane, and the edge points, of four frames,
    queued with no synchronisation on a pipelined context: the chains include/hipcanny.h documents as needing none.  Closing joins
    edges: fewer components behind it than before."""
    P = _params(w=130, h=67, mode="O", pipeline=True)
    with DS.Executor(P, oracle, "the real chain, closed") as e:
        e.queue(dict(kind="canny", f0=0, n=4, out=0, low=DS.CANNY_THR[3][0], high=DS.CANNY_THR[3][1], aperture=3, l2=0))
        edges = _region(e.model, 0, 4).copy()
        for st in (_morph(("whole", 0), 4, into=1), _components(("whole", 1), 4, P), _dist(("whole", 1), 4, P, near="side", swords=3), _points(("whole", 1), 4, P=P)):
            e.queue(st)
        c = e.model.counters
        assert c["morph_overlap_in"] == 1 and c["morph_read_by_a_later_step"] == 3 and c["dist_of_morph_output"] == 1 and c["dist_side_by_side"] == 1 and not e.model.pending, c
        e.check()
        assert e.continued_runs() == 1
        before, after = DS.CC.connected_components(edges, 8, 0)[1].tolist(), _component_counts(e.model, 0, 4)
        assert all(b >= a > 1 for b, a in zip(before, after)) and sum(before) > sum(after), (before, after)
        assert _point_counts(e.model, 0, 4) == [int(np.count_nonzero(m)) for m in _region(e.model, 1, 4)] and c["dist_without_features"] == 0, c


def test_distances_without_features_then_with(oracle):
    """HC_DT_TO_ZERO on a view of the arena's fill (no zero byte: HC_DT_NONE / +inf and -1), checked; then the same calls again, each
    followed at once by HC_DT_TO_NONZERO of a pending run's maps into the same planes, whose first frame still holds what the
    call before left there."""
    P = _params()
    none = lambda dtype, dslot: _dist(("before", 0), 1, P, target=api.DT_TO_ZERO, dtype=dtype, dslot=dslot, near="side")
    some = lambda dtype, dslot: _dist(("whole", 0), 4, P, dtype=dtype, dslot=dslot, near="side")
    with DS.Executor(P, oracle, "distances without features, then with") as e:
        for st in (_run(0, 0), none(api.DT_SQUARED_I32, 0), none(api.DT_F32, 1)):
            e.queue(st)
        e.check()
        c, L = e.model.counters, e.L
        assert c["dist_without_features"] == 2 and c["dist_maps_mixed"] == 0 and c["adjacent"] == 2, c   # (both views end where the pending output begins: its run stays in flight)
        for dtype, dslot, want in ((np.int32, 0, api.DT_NONE), (np.float32, 1, np.inf)):
            (dn, doff, dp, dfs), near = DS.dist_views(L, none(0, dslot))
            assert (e.model.get(dn, doff, dp, dfs, 1, 4 * P["w"]).view(dtype) == want).all() and (e.model.get(*near, 1, 4 * P["w"]).view(np.int32) == -1).all()
        for st in (_run(0, 0), none(api.DT_SQUARED_I32, 0), some(api.DT_SQUARED_I32, 0), none(api.DT_F32, 1), some(api.DT_F32, 1)):
            e.queue(st)
        assert c["dist_overlap_map"] == 1 and c["dist_without_features"] == 4 and c["dist_maps_mixed"] == 2, c
        e.check()
        assert e.continued_runs() == 2
