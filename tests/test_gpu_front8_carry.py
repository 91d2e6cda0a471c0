"""k_front8, mono full-strip instances: the fix-up chain reads its 25 taps from the caller's frame instead of an LDS ring of
input rows, the blur ring holds 16 rows, and a queued NMS entry may wait one window for a full batch (front8.hip, window).

What can go wrong: a tap read outside the caller's W x H view (left / right of the row, above / below the frame, in the
pitch padding); a ring slot that no longer holds the blur row an entry reads; an entry that waits past the last window of
its run, or across a hand-over to the dense loop; a pair of entries split over two batches.  Every case runs on a pitched
view at a 4-byte offset inside an allocation whose every other byte is 0xFF -- a tap from outside the view changes the blur
-- pipelined (provisional map) and not, and compares the blur rows and bit planes the front kernel left (hc_debug_tap) and
the final maps with the oracle, bit for bit."""
import numpy as np
import pytest

from cudacam_amd import api, synth

from test_gpu_parity import _diff

pytestmark = pytest.mark.gpu

LOW, HIGH = 10, 40
LEAD = 512 + 4   # the view starts 4 bytes past a 512-byte boundary


def _round_up(x, m):
    return (x + m - 1) // m * m


def _check(oracle, frames, what, pipeline, chunk=0, dense=-1, wpb=None):
    import torch
    frames = np.ascontiguousarray(frames)
    n, h, w = frames.shape
    pitch = _round_up(w, 8) + 40
    fs = pitch * h + 24
    arena = np.full(LEAD + n * fs + pitch + 64, 0xFF, np.uint8)
    for f in range(n):
        rows = arena[LEAD + f * fs: LEAD + f * fs + pitch * h].reshape(h, pitch)
        rows[:, :w] = frames[f]
    stages = [oracle.canny_r(f, LOW, HIGH, stages=True) for f in frames]
    want = oracle.canny_r_batch(frames, LOW, HIGH)
    d_in = torch.from_numpy(arena).cuda()
    d_out = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with api.Context(w, h, 1, n) as ctx:
        ctx.set_thresholds(LOW, HIGH)
        ctx.set_option(api.OPT_FRONT_HALF, 0)   # the full-strip form at every width
        ctx.set_option(api.OPT_FRONT_DENSE, dense)
        ctx.set_option(api.OPT_PIPELINE, pipeline)
        ctx.set_option(api.OPT_DEBUG_TAPS, 1)
        if wpb is not None:
            ctx.set_option(api.OPT_FRONT_WPB, wpb)
        if chunk:
            ctx.set_tuning(chunk, 0)
        ctx.run_device(d_in.data_ptr() + LEAD, pitch, fs, d_out.data_ptr(), w, w * h, n)
        ctx.sync()
        staged_in, _, form = ctx.last_run_info()
        assert not staged_in and form == 2, f"{what}: input staged {staged_in}, front form {form}"
        blur, thr = ctx.debug_tap(api.TAP_BLUR, n), ctx.debug_tap(api.TAP_THRESH, n)
    got = d_out.cpu().numpy()
    for f in range(n):
        _diff(blur[f], stages[f]["blur"], f"{what}, frame {f}: blur")
        _diff(thr[f], stages[f]["thresh"], f"{what}, frame {f}: bit planes")
        _diff(got[f], want[f], f"{what}, frame {f}: edges")


# ---- content ----------------------------------------------------------------------------------------------------------
def _dots(w, h, seed):
    """A few isolated 3 x 3 steps on a gradient (not flat: no fix-up overflow): every window queues far fewer than 64
    entries, everything is carried and the run's last window has to flush it."""
    yy, xx = np.mgrid[0:h, 0:w]
    img = ((xx * 3 + yy * 5) % 23 + 60).astype(np.uint8)   # steps of 3 and 5 per pixel: gradients below the low threshold
    rng = np.random.default_rng(seed)
    for _ in range(max(2, w * h // 1500)):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        img[max(0, y - 1): y + 2, max(0, x - 1): x + 2] = 200
    return img


def _columns(w, h, period):
    """Vertical bars every `period` columns: each row queues two to four half-lanes per bar, the same ones in every row."""
    yy, xx = np.mgrid[0:h, 0:w]
    img = ((xx + 2 * yy) % 7 + 50).astype(np.uint8)
    img[:, (xx[0] % period) < period // 2] += 120
    return img


def _over(top, bottom, cut):
    img = top.copy()
    img[cut:] = bottom[cut:]
    return img


def _flat_areas(w, h, seed):
    """Constant areas (every pixel of them has S % 159 == 0: the fix-up queue overflows, the window is recomputed) around a block of noise."""
    img = np.full((h, w), 131, np.uint8)
    nz = synth.noise(w, h, seed)
    img[h // 3: h // 3 + 5, w // 4: w // 4 + 40] = nz[h // 3: h // 3 + 5, w // 4: w // 4 + 40]
    img[:, w // 2:] = 17
    return img


def _mixed(w, h, seed):
    return np.stack([synth.noise(w, h, seed), _dots(w, h, seed + 1), _columns(w, h, 62), _flat_areas(w, h, seed + 2)])


# ---- widths: a strip border, and a frame border inside a lane, at every position the taps reach ------------------------------
# (W = 0 and 7 mod 8: the right-hand taps lie beyond round_up(W, 8); 496 / 497 / 503 / 504: a second strip of 0, 1, 7, 8 columns;
# 1000: three strips)
WIDTHS = [8, 9, 15, 16, 17, 495, 496, 497, 503, 504, 1000]


@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("w", WIDTHS)
def test_widths(oracle, w, pipeline):
    _check(oracle, _mixed(w, 22, 3 * w), f"{w}x22, pipeline {pipeline}", pipeline)
    _check(oracle, _mixed(w, 22, 3 * w), f"{w}x22, one run, pipeline {pipeline}", pipeline, chunk=122)


# ---- heights: runs of 1, 2, 3, 4 and 5 windows (a run of H rows has (H + 9) / 6 windows), and frames cut into several runs -----
# (chunk 122 >= H: one run.  chunk 20: runs of 4 windows -- 50 rows are 20 + 20 + 10.  chunk 0: the planner's own cut, which
# for a few small frames is runs of two windows, cut_front8_runs in host_plan.h)
HEIGHTS = [(2, 122), (3, 122), (8, 122), (9, 122), (14, 122), (16, 122), (22, 122), (50, 20), (50, 14), (50, 0)]


@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("h,chunk", HEIGHTS)
def test_heights(oracle, h, chunk, pipeline):
    _check(oracle, _mixed(520, h, 7 * h + chunk), f"520x{h}, runs of {chunk}, pipeline {pipeline}", pipeline, chunk=chunk)


# ---- full batches plus a carried rest -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("period", [40, 62, 124])
def test_edge_columns(oracle, period, pipeline):
    """992 columns, bars every 124 / 62 / 40: about 5, 10 and 16 half-lanes per row and strip, 32 to 100 a window -- windows
    that carry everything, that take one full batch and carry the rest, and that take a batch at mid-window too."""
    frames = np.stack([_columns(992, 46, period), _columns(992, 46, period)[:, ::-1].copy()])
    for chunk in (0, 20, 122):
        _check(oracle, frames, f"bars every {period}, runs of {chunk}, pipeline {pipeline}", pipeline, chunk=chunk)


# ---- a carry meets the hand-over into and out of the dense loop ---------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("dense", [0, 1, -1], ids=["never", "always", "auto"])
def test_noise_next_to_sparse_rows(oracle, dense, pipeline):
    """Noise below sparse rows and the reverse, the seam at rows that fall early, in the middle and late in a window; runs of
    2 windows (the planner's), 3, 4 and one run -- the seam also falls on the first window of a run that does not start at
    row 0, which is judged on the two rows it owns."""
    w, h = 992, 62
    nz, sp = synth.noise(w, h, 5), _columns(w, h, 124)
    frames = np.stack([_over(sp, nz, 20), _over(nz, sp, 20), _over(sp, nz, 29), _over(nz, sp, 33), _over(_dots(w, h, 9), nz, 40)])
    for chunk in (0, 14, 20, 122):
        _check(oracle, frames, f"noise / sparse, dense {dense}, runs of {chunk}, pipeline {pipeline}", pipeline, chunk=chunk, dense=dense)


# ---- the fix-up queue overflows: the whole window from global taps --------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("w", [17, 504, 1000])
def test_flat_frames(oracle, w, pipeline):
    frames = np.stack([synth.flat(w, 16, 255), synth.flat(w, 16, 1), _flat_areas(w, 16, w)])
    _check(oracle, frames, f"flat {w}x16, pipeline {pipeline}", pipeline)
    _check(oracle, frames, f"flat {w}x16, one run, pipeline {pipeline}", pipeline, chunk=122)


# ---- pure noise, and the workgroup forms ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("dense", [0, 1, -1], ids=["never", "always", "auto"])
def test_pure_noise(oracle, dense, pipeline):
    frames = np.stack([synth.noise(1000, 40, 21), synth.noise(1000, 40, 22)])
    _check(oracle, frames, f"noise, dense {dense}, pipeline {pipeline}", pipeline, dense=dense)
    _check(oracle, frames, f"noise, dense {dense}, runs of 20, pipeline {pipeline}", pipeline, chunk=20, dense=dense)


@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("wpb", [1, 4])
def test_waves_per_workgroup(oracle, wpb, pipeline):
    frames = np.stack([synth.natural(1000, 64, 31), _over(synth.natural(1000, 64, 32), synth.noise(1000, 64, 33), 30), _columns(1000, 64, 62)])
    for chunk in (0, 122):
        _check(oracle, frames, f"wpb {wpb}, runs of {chunk}, pipeline {pipeline}", pipeline, chunk=chunk, wpb=wpb)
