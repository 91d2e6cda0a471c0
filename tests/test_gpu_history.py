"""Run SEQUENCES on one context whose content, batch size and entry point change from run to run.

How libhipcanny queues a run's hysteresis follows what the earlier runs of the context observed (hipcanny.hip:
hyst_need_rows, wl_prev, last_work_launches / hyst_lists_last, hyst_obs, big_slots, dl_stale ...).  A prediction that is wrong
may cost time, never a pixel: the flag of the last queued launch and the host-side continuation guarantee that.  The other
GPU tests open a context per case or send it the same batch again and again, so they only see histories that agree with the
content.  Here every sequence is scripted to make the history wrong in one direction after the other, every map of every
run is compared with the oracle (tests/fuzz_sequences.py, class Sequence), and every sequence ends by asserting through
hc_last_hysteresis_schedule / hc_last_hysteresis_info that it really reached the schedules it is about."""
import os
import subprocess
import sys
from itertools import permutations

import pytest

from cudacam_amd import api
import fuzz_sequences as FS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

ZERO, FLAT, NOISE, NATURAL, WOBBLE, VCHAIN, SPARSE = range(7)   # pool indices: FS.KINDS in order


def _pool(w, h):
    return [FS.make_frame(k, w, h, 11 + i) for i, k in enumerate(FS.KINDS)]


def _show(s, title):
    print(f"\n-- {title}: {s.run_no} runs, {s.maps_compared} maps compared; runs / continued / launches with work / launches queued: {s.ctx.hysteresis_totals()}")
    for e in s.log:
        print("   run %(run)3d %(what)-28s K %(launches)2d work %(work)3d cont %(cont)d lists %(lists)d loop %(loop)d hist_grid %(hist_grid)5d longest %(longest)5d "
              "overflows %(overflows)2d tiles %(tiles)5d tile %(tile_rows)dx%(waves)d panels %(panels)d frames %(frames)d slots %(slots)d" % e)


def _rises_and_falls(log):
    """launches-with-work moved by more than the +-30 % of hipcanny.hip's `observe` reset, both ways, between consecutive logged runs"""
    up = any(b["work"] * 10 > a["work"] * 13 + 20 for a, b in zip(log, log[1:]))
    down = any(b["work"] * 10 < a["work"] * 7 - 20 for a, b in zip(log, log[1:]))
    return up, down


def test_small_frames_one_call_at_a_time(oracle):
    """300 x 1400, one to three frames per synchronous call: the looping launch (k_hyst_loop), K capped at need + 2.
    quiet -> chain (K = 4 queued, 12 needed: continuation) -> chain (estimate followed: none) -> quiet -> chain before the
    estimate has decayed (none) -> 50 quiet runs (32 rows a run) -> chain after (continuation again); the batch size
    changes with the content fixed; an empty frame, a chain and noise side by side in every order; process, run_device
    into two buffers, hysteresis_device (all candidates + one seed directly after an empty map), download_begin .. another
    run .. download_end; thresholds and saturating NMS changed between runs.
    Measured on an MI355X: 451 runs, 504 maps; nine of the runs continued from the host; the nine scripted tests of this file
    take 6 s together."""
    w, h = 300, 1400
    with FS.Sequence(oracle, w, h, _pool(w, h), max_batch=3, nbuf=2, thr_pool=FS.thr_maps(w, h)) as s:
        s.device([ZERO])
        s.device([VCHAIN])                       # history says "nothing to do"
        s.device([VCHAIN])
        s.process([ZERO, ZERO])
        s.device([VCHAIN, WOBBLE])               # before the estimate has decayed
        for _ in range(50):
            s.device([FLAT])
        s.device([VCHAIN])                       # ... and after
        for n in (1, 3, 2, 1, 3):                # batch size changes, content fixed
            s.device([WOBBLE] * n)
        for order in permutations((ZERO, VCHAIN, NOISE)):
            s.device(list(order))
            s.process(list(order)[::-1])
        s.hyst([0])                              # an empty map ...
        s.hyst([3])                              # ... then all candidates, one seed
        s.hyst([1, 0, 2])
        s.device([NATURAL], sync=False)
        s.hyst([1], sync=False)
        s.flush()
        s.thresholds(30, 90)
        s.device([NOISE, VCHAIN], sync=False)
        s.thresholds(10, 40)
        s.device([VCHAIN, NOISE], sync=False)    # two runs in flight with different thresholds
        s.flush()
        s.option(api.OPT_NMS_SATURATE, 1)
        s.download_split([NOISE, VCHAIN, ZERO], between=lambda: s.device([WOBBLE], sync=False))
        s.option(api.OPT_NMS_SATURATE, 0)

        def calm():   # the estimate decays by 32 rows a run: back to the floor of four launches
            for _ in range(50):
                s.device([ZERO])

        # a run whose download is already queued is continued from the host -- inside another entry point, or in
        # hc_download_end itself: the maps must be copied again (dl_stale)
        for between in (lambda: s.hyst([0], sync=False), lambda: s.device([ZERO], sync=False), s.ctx.sync, None):
            calm()
            before = s.ctx.hysteresis_totals()[1]
            s.download_split([VCHAIN, ZERO], between=between)
            assert s.ctx.hysteresis_totals()[1] == before + 1, "the run being downloaded was not continued from the host"
        s.option(api.OPT_PIPELINE, 1)
        for k in range(6):
            s.device([(ZERO, VCHAIN, NOISE, WOBBLE)[k % 4]] * (1 + k % 3), sync=k % 2 == 1)
        s.process([VCHAIN, ZERO, WOBBLE])
        for between in (lambda: s.device([ZERO, NOISE], sync=False), lambda: s.hyst([0], sync=False), None):   # the same with HC_OPT_PIPELINE on
            for _ in range(50):
                s.device([ZERO], sync=False)
            s.flush()
            before = s.ctx.hysteresis_totals()[1]
            s.download_split([VCHAIN, ZERO], between=between)
            assert s.ctx.hysteresis_totals()[1] >= before + 1, "the pipelined run being downloaded was not continued from the host"
        s.option(api.OPT_PIPELINE, 0)
        s.device([VCHAIN])
        s.flush()
        _show(s, "small frames")
        loop = [e for e in s.log if e["loop"]]
        assert any(e["cont"] for e in loop), "no run of the looping launch needed the continuation"
        assert any(not e["cont"] for e in loop), "every run of the looping launch needed the continuation"
        assert any(e["launches"] == 4 and e["cont"] for e in s.log), "no run was queued with the floor of need + 2 launches and needed more"
        assert all(_rises_and_falls(s.log)), "launches with work did not both rise and fall by more than 30 %"
        assert any(not e["loop"] for e in s.log)
        assert s.ctx.hysteresis_totals()[1] >= 6


def test_1080p_lists_come_and_go(oracle):
    """1080p, 4 frames per call and 128 per pipelined run (from 122 frames on the tiles are 64 rows high): one-panel streams
    take worklists from launch 1 once a run needed 20 launches, keep them down to 14, and otherwise run the mixed schedule (a
    workgroup per tile, lists from launch 3) when pipelined.
    Measured on an MI355X: 45 runs, 2043 maps; WOBBLE needs 24 launches with 64-row tiles and 21 with 128-row tiles, after which
    the 128-frame runs move to 128-row tiles (hyst_obs) and VCHAIN needs 10 -- so the hold (14 .. 19 launches) is reached with
    the four-frame runs and the three milder wobble frames.  (The log, and so the assertions at the end, cover the runs that
    completed one at a time: see fuzz_sequences.Sequence.)"""
    w, h = 1920, 1080
    # three more frames whose edge crosses the tile boundary at row 128 less often than WOBBLE's: between 14 and 19 launches
    mild = [FS.wobble(w, h, 128, 20, w // k) for k in (9, 11, 13)]
    with FS.Sequence(oracle, w, h, _pool(w, h) + mild, max_batch=128, nbuf=4) as s:
        s.device([ZERO] * 4)
        s.device([WOBBLE, ZERO, NATURAL, VCHAIN])
        s.device([NATURAL] * 4)
        s.process([VCHAIN, NOISE, ZERO, WOBBLE])
        s.option(api.OPT_PIPELINE, 1)
        assert s.ctx.pipeline_depth(128) == 4
        for n in (128, 4):   # 128 frames: 64-row tiles (17 row tiles); 4 frames: 128-row tiles
            s.device([ZERO] * n)
            s.device([WOBBLE] * n)                   # >= 20 launches: the next run takes lists
            s.device([VCHAIN] * n)                   # lists (measured: 10 launches, the tiles have grown to 128 rows)
            s.device([VCHAIN, ZERO] * (n // 2))
            s.device([NATURAL] * n)
            s.device([NATURAL, SPARSE] * (n // 2))   # the mixed schedule again
            s.device([ZERO] * n)
            for order in permutations((ZERO, WOBBLE, NOISE)):
                s.device((list(order) * n)[:n], sync=False)   # four in flight, each chain on a stream of its own
            s.flush()
        for m in (7, 8, 9):                          # four frames per run: 128-row tiles, no taller shape to move to
            s.device([WOBBLE] * 4)                   # >= 20 launches
            s.device([m] * 4)                        # lists
            s.device([m, ZERO] * 2)                  # kept if the run before needed 14 .. 19
            s.device([NATURAL] * 4)
        s.thresholds(40, 120)
        s.option(api.OPT_FRONT_MX, 1)
        s.device([NATURAL, WOBBLE, NOISE, ZERO] * 32, sync=False)
        s.option(api.OPT_FRONT_MX, 0)
        s.option(api.OPT_FRONT_WPB, 1)
        s.device([WOBBLE] * 128, sync=False)
        s.thresholds(10, 40)
        s.option(api.OPT_FRONT_WPB, 4)
        s.device([WOBBLE] * 7)
        s.flush()
        _show(s, "1080p")
        log = s.log
        assert any(e["lists"] == 2 for e in log), "no run took the mixed schedule"
        assert any(e["lists"] == 1 for e in log), "no run took worklists from launch 1"
        assert any(b["lists"] == 1 and 14 <= a["work"] < 20 for a, b in zip(log, log[1:]) if b["run"] == a["run"] + 1), "lists were never kept by the 14-launch hold"
        assert any(b["lists"] != 1 and a["lists"] == 1 for a, b in zip(log, log[1:])), "lists were never given up again"
        assert any(e["cont"] for e in log) and any(not e["cont"] and e["work"] >= 14 for e in log)
        assert all(_rises_and_falls(log))


def _frames_for_tiles(w, h, piped, target):
    """frames per run so that the run has at least `target` tiles -- from the diagnostic, not from a guess of the tile shape
    (which itself follows the batch size)"""
    n = 1
    for _ in range(4):
        with api.Context(w, h, 1, n) as ctx:
            import torch
            z = torch.zeros((n, h, (w + 7) // 8 * 8), dtype=torch.uint8, device="cuda")
            o = torch.zeros_like(z)
            torch.cuda.current_stream().synchronize()
            if piped:
                ctx.set_option(api.OPT_PIPELINE, 1)
            ctx.run_device(z.data_ptr(), z.shape[2], z.shape[2] * h, o.data_ptr(), z.shape[2], z.shape[2] * h, n)
            ctx.sync()
            tiles = ctx.hysteresis_schedule()["tiles"]
        if tiles >= target:
            return n
        n = -(-target * n // tiles)
    raise AssertionError(f"{w}x{h}: no batch size gives {target} tiles")


@pytest.mark.parametrize("w,h,piped", [(4500, 300, False), (8184, 70, True)])
def test_wide_frames_grids_sized_by_the_last_run(oracle, w, h, piped):
    """Frames of four 2048-column panels, enough of them per run for 4200 tiles or more (4500 x 300: 350 frames of 12 tiles;
    8184 x 70 pipelined: 525 of 8), so that max(2048, 2 * wl_prev[k] + 256) is what sizes the grids of the list launches.
    quiet -> noise (lists; grid 2048 from the quiet run's empty lists, 80 % of the tiles listed: entries beyond the grid are
    handed on) -> noise (more than 60 % listed last time: a workgroup per tile) -> sparse long edges (lists again) -> noise
    (grid from the sparse run's short lists) -> chains; then the batch size moves (wl_prev belongs to another tile count:
    no history grid) and comes back; an empty frame, a chain and noise side by side in every order.
    Measured on an MI355X: 4500 x 300: 350 frames per run (12 tiles a frame), 22 runs, 6664 maps; the noise run after the quiet
    one serves lists of 4200 entries with grids of 2048 in three launches.  8184 x 70 pipelined: 1050 frames (4 tiles a frame: the
    tiles are 128 rows high below 128 K rows per run), 22 runs, 19853 maps."""
    n = _frames_for_tiles(w, h, piped, 4200)
    assert n <= 1200
    with FS.Sequence(oracle, w, h, _pool(w, h), max_batch=n, nbuf=2, thr_pool=FS.thr_maps(w, h)) as s:
        if piped:
            s.option(api.OPT_PIPELINE, 1)
        s.device([ZERO] * n)
        s.device([NOISE] * n)
        s.device([NOISE] * n)
        s.device([SPARSE] * n)
        s.device([NOISE] * n)
        s.device([WOBBLE] * n)
        s.device([ZERO] * n)
        s.device([WOBBLE, SPARSE] * (n // 2))
        for m in (n // 2, n, n // 3, n):          # wl_prev_tiles == wl_stride flips; n below and above what wl_prev was recorded for
            s.device([WOBBLE, NATURAL, ZERO] * (m // 3))
        s.device([SPARSE] * n)
        for order in permutations((ZERO, WOBBLE, NOISE)):
            s.device((list(order) * n)[:n], sync=False)
        s.flush()
        s.hyst([0] * min(n, 40))
        s.hyst([3, 1] * min(n // 2, 20))
        s.device([NOISE, ZERO] * (n // 2))
        s.flush()
        _show(s, f"wide frames {w}x{h}")
        log = s.log
        assert all(e["panels"] == 4 for e in log)
        assert max(e["tiles"] for e in log) >= 4200
        # (pipelined runs start a workgroup per tile in launches 0 to 2 and end on lists -- the mixed schedule -- where plain runs keep the workgroup per tile)
        assert any(e["lists"] == 1 for e in log) and any(e["lists"] == (2 if piped else 0) for e in log), "not both the list and the per-tile scheme"
        assert any(e["hist_grid"] > 0 and e["overflows"] > 0 and e["longest"] > e["hist_grid"] for e in log), "no launch had a list longer than its history-sized grid"
        assert any(e["lists"] == 1 and e["hist_grid"] == 0 and e["run"] > 0 for e in log), "no list run without a history grid (batch size changed)"
        assert any(e["cont"] for e in log) and any(not e["cont"] and e["work"] > 1 for e in log)
        assert all(_rises_and_falls(log))


def test_big_batches_content_changes_while_the_third_slot_comes_and_goes(oracle):
    """4000 frames of 640 x 200 per pipelined run (0.51 G pixels: the two- / three-slot ring).  The ring's size follows event
    timestamps, so it is driven by hand (HC_OPT_PIPELINE_SLOTS 20 / 21, as test_big_batches_take_a_third_slot... does) and only
    what was forced is asserted; what is new is that the content changes while the third slot is on trial, adopted, and given
    back -- and k_front8's workgroup size (HC_OPT_FRONT_WPB) with it.
    The log (runs that completed one at a time) holds the few synchronous runs only: that three slots were in use is asserted
    through hc_pipeline_slots_in_use after each burst, not through the log.
    Measured on an MI355X: 80 runs, 314100 maps, nine runs continued from the host.  This sequence is where the wrong maps of
    test_first_run_on_a_slot_allocated_with_runs_in_flight were first seen."""
    w, h, n = 640, 200, 4000
    with FS.Sequence(oracle, w, h, _pool(w, h), max_batch=n, nbuf=3) as s:
        s.option(api.OPT_PIPELINE, 1)
        contents = [[ZERO], [WOBBLE, NATURAL], [NOISE], [VCHAIN, ZERO, NOISE], [SPARSE], [WOBBLE]]
        step = [0]

        def runs(k):
            for _ in range(k):
                c = contents[(step[0] // 2) % len(contents)]   # the content changes every second run
                step[0] += 1
                s.device((c * n)[:n], sync=False)
            s.flush()
            return s.ctx.pipeline_slots_in_use()

        s.device([ZERO] * n)
        s.device([WOBBLE] * n)                  # six launches queued, thirty needed
        s.device([WOBBLE] * n)
        runs(6)
        s.option(api.OPT_PIPELINE_SLOTS, 20)    # every chain counts as outlasting the next front kernel
        assert runs(8) == 3, "third slot not taken on trial"
        s.option(api.OPT_FRONT_WPB, 1)
        assert runs(8) == 3, "third slot not kept"
        s.option(api.OPT_PIPELINE_SLOTS, 21)    # every chain counts as ending first
        s.option(api.OPT_FRONT_WPB, 4)
        assert runs(26) == 2, "third slot not given back after sixteen runs"
        assert s.ctx.front_waves_per_workgroup() == 4
        s.option(api.OPT_PIPELINE_SLOTS, 20)
        s.option(api.OPT_FRONT_WPB, 1)
        assert runs(8) == 3
        assert s.ctx.front_waves_per_workgroup() == 1
        s.option(api.OPT_PIPELINE_SLOTS, 21)
        assert runs(16) == 2, "a trial that does not pay was not ended"
        s.option(api.OPT_FRONT_WPB, -1)
        s.device([WOBBLE] * n)
        s.device([ZERO] * n)
        s.device([VCHAIN] * (n // 2))
        s.device([NOISE] * 100)                 # a small batch on the same context: the four-slot ring
        assert s.ctx.pipeline_slots_in_use() == 4
        s.device([WOBBLE] * n)
        s.flush()
        _show(s, "big batches")
        assert any(e["cont"] for e in s.log) and any(not e["cont"] for e in s.log)
        assert {e["slots"] for e in s.log} >= {2, 4}


def test_first_run_on_a_slot_allocated_with_runs_in_flight(oracle):
    """Regression.  Slots 1 .. 3 of a context are allocated inside the run that first uses them -- for a big batch when the
    ring grows from two slots to three, with two runs in flight.  Their bit planes were cleared with hipMemset, i.e. on the
    null stream: the call returns at once (measured: 4 - 40 us for 1 GiB), the context's non-blocking streams do not wait
    for that stream, and the clear runs behind whatever else the process has queued there -- torch's default stream IS the null
    stream.  With 13 ms of such work in flight the clear lands after the front kernel of the slot's first run and wipes the
    planes it has just filled (probe: every byte a non-blocking stream wrote after the call read 0 afterwards).  First seen as
    one run in five of the big-batch sequence above: run 14, 4000 wobble frames, 3673 maps with the strong pixels only (hip 0,
    oracle 255).  The clear is now queued on the context stream and waited for (alloc_slot_parts).
    Here: two slots, runs in flight, the ring grows (HC_OPT_PIPELINE_SLOTS 3), the caller has work on the null stream, and the
    third run -- chains in every frame, so that missing candidates show -- is the first on the new slot; then the same for
    slots 2 and 3 of the four-slot ring of small batches.  Fails on every repeat with the old clear."""
    import torch
    w, h = 640, 200
    pool = _pool(w, h)
    busy = torch.zeros(1 << 30, dtype=torch.uint8, device="cuda")

    def load():
        for _ in range(40):
            busy.add_(1)

    for n in (4000, 64):
        for _ in range(2):
            with FS.Sequence(oracle, w, h, pool, max_batch=n, nbuf=4) as s:
                s.option(api.OPT_PIPELINE, 1)
                s.null_stream_load = load
                if n == 4000:
                    s.option(api.OPT_PIPELINE_SLOTS, 2)
                    s.device([SPARSE] * n, sync=False)
                    s.device([SPARSE] * n, sync=False)
                    s.flush()
                    s.option(api.OPT_PIPELINE_SLOTS, 3)
                    s.device([NOISE] * n, sync=False)
                    s.device([WOBBLE] * n, sync=False)
                    s.device([WOBBLE, VCHAIN] * (n // 2), sync=False)   # the first run on slot 2
                    s.flush()
                    assert s.ctx.pipeline_slots_in_use() == 3
                else:   # small batches: slots 2 and 3 are first used by the third and fourth run in flight
                    for c in ([NOISE], [WOBBLE], [WOBBLE, VCHAIN], [VCHAIN, NATURAL]):
                        s.device((c * n)[:n], sync=False)
                    s.flush()
                    assert s.ctx.pipeline_slots_in_use() == 4
            torch.cuda.synchronize()


def test_mode_o_history(oracle):
    """Mode O (cv::Canny semantics: its own front kernels, and a tile-height history of its own in hyst_obs) through the same
    wrong histories on one context, 300 x 1400 and thresholds 50 / 150 (a step of 20 grey levels gives |dx| + |dy| = 80: weak;
    the graded head is strong): quiet -> chain (continuation) -> chain -> quiet -> chain before the estimate has decayed -> 50
    quiet runs -> chain after; the batch size moves; an empty frame, a chain and noise side by side in every order; process,
    run_device, hysteresis_device, download_begin .. run .. download_end, plain and pipelined; L2 gradient and thresholds changed
    between runs."""
    w, h = 300, 1400
    with FS.Sequence(oracle, w, h, _pool(w, h), max_batch=3, mode="O", nbuf=2, thr_pool=FS.thr_maps(w, h)) as s:
        assert (s.lo, s.hi) == (50, 150)
        s.device([ZERO])
        s.device([VCHAIN])
        s.device([VCHAIN])
        s.process([ZERO, ZERO])
        s.device([VCHAIN, WOBBLE])
        for _ in range(50):
            s.device([FLAT])
        s.device([VCHAIN])
        for n in (1, 3, 2, 1, 3):
            s.device([WOBBLE] * n)
        for order in permutations((ZERO, VCHAIN, NOISE)):
            s.device(list(order))
            s.process(list(order)[::-1])
        s.hyst([0])
        s.hyst([3])
        s.option(api.OPT_L2_GRADIENT, 1)
        s.device([VCHAIN, NOISE, NATURAL])
        s.thresholds(30, 200)
        s.device([NOISE, VCHAIN], sync=False)
        s.thresholds(50, 150)
        s.option(api.OPT_L2_GRADIENT, 0)
        for piped in (0, 1):
            s.option(api.OPT_PIPELINE, piped)
            for between in (lambda: s.device([ZERO], sync=False), lambda: s.hyst([0], sync=False), None):
                for _ in range(50):
                    s.device([ZERO], sync=not piped)
                s.flush()
                before = s.ctx.hysteresis_totals()[1]
                s.download_split([VCHAIN, ZERO], between=between)
                assert s.ctx.hysteresis_totals()[1] >= before + 1, "the run being downloaded was not continued from the host"
            for k in range(8):
                s.device([(ZERO, VCHAIN, NOISE, WOBBLE)[k % 4]] * (1 + k % 3), sync=k % 2 == 1)
        s.flush()
        _show(s, "mode O")
        loop = [e for e in s.log if e["loop"]]
        assert any(e["cont"] for e in loop), "no run of the looping launch needed the continuation"
        assert any(not e["cont"] for e in loop), "every run of the looping launch needed the continuation"
        assert any(not e["cont"] and e["work"] >= 6 for e in s.log), "no chain was finished by the queued launches"
        assert any(not e["loop"] for e in s.log)
        assert all(_rises_and_falls(s.log)), "launches with work did not both rise and fall by more than 30 %"


def test_front_forms_toggled_between_runs(oracle):
    """640 x 480 (k_front8 takes its half-strip form here on its own): HC_OPT_FRONT_HALF 0 / 1 / -1, HC_OPT_FRONT_MX and
    HC_OPT_FRONT_WPB changed between runs of one context, plain and pipelined, while the content moves between quiet frames,
    chains and noise; the front form each run took is read back (hc_last_run_info: 2 k_front8, 4 its half-strip form, 5 k_front_mx)."""
    w, h = 640, 480
    with FS.Sequence(oracle, w, h, _pool(w, h), max_batch=4, nbuf=4) as s:
        forms = set()
        for piped in (0, 1):
            s.option(api.OPT_PIPELINE, piped)
            for half, mx, wpb, content in ((0, 0, -1, [ZERO] * 4), (1, 0, 1, [VCHAIN, NOISE, ZERO]), (-1, 0, 4, [WOBBLE] * 4), (0, 1, 1, [VCHAIN] * 2),
                                           (1, 1, -1, [NOISE, WOBBLE, ZERO, VCHAIN]), (1, 0, 4, [ZERO]), (0, 0, 1, [WOBBLE, VCHAIN]), (-1, 0, -1, [NATURAL] * 4)):
                s.option(api.OPT_FRONT_HALF, half)
                s.option(api.OPT_FRONT_MX, mx)
                s.option(api.OPT_FRONT_WPB, wpb)
                s.device(content)
                forms.add(s.ctx.last_run_info()[2])
                s.device(content[::-1], sync=False)
                s.device([ZERO] * len(content), sync=False)
                s.flush()
        _show(s, "front forms")
        assert forms >= {2, 4, 5}, f"front forms seen: {forms}"
        assert any(e["cont"] for e in s.log) and any(not e["cont"] for e in s.log)


def test_header_documented_refusals():
    """What these sequences never generate because the header documents it as refused: HC_E_ARG and the message."""
    with api.Context(64, 64, 1, 2) as ctx:
        import torch
        z = torch.zeros((3, 64, 64), dtype=torch.uint8, device="cuda")
        for call, msg in ((lambda: ctx.run_device(z.data_ptr(), 64, 4096, z.data_ptr(), 64, 4096, 3), "nframes out of range"),
                          (lambda: ctx.hysteresis_device(z.data_ptr(), 64, 4096, z.data_ptr(), 64, 4096, 3), "nframes out of range"),
                          (lambda: ctx.set_option(api.OPT_PER_CHANNEL, 1), "HC_OPT_PER_CHANNEL needs a 3-channel context"),
                          (lambda: ctx.set_option(api.OPT_PIPELINE_SLOTS, 5), "HC_OPT_PIPELINE_SLOTS")):
            with pytest.raises(api.HipCannyError) as e:
                call()
            assert "error -1:" in str(e.value) and msg in str(e.value)
        assert ctx.hysteresis_schedule() == dict.fromkeys(api.SCHEDULE_FIELDS, 0)   # nothing ran


@pytest.mark.parametrize("seed", [1, 2])
def test_random_sequences_match_oracle(oracle, seed):
    """tests/fuzz_sequences.py: per case one context and 8-20 runs, everything drawn per run.  300 cases per seed: measured on an
    MI355X 85 to 110 s per seed, oracle included (about 4600 runs and 18000 maps; profiles/r06_history/fuzz_sequences.txt) -- well
    inside the 600 s of the subprocess, and less than half of it even if the oracle were all of it."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_sequences.py"), "300", str(seed)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " 0 mismatches" in out.stdout
