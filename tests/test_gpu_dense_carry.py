"""k_front8's dense path, warm form: a dense window that follows another dense window of the same run starts from what
that window left in registers -- the S2 of its last two Sobel rows with their halo entries, the newest Sobel sums and the
d / s of its last two blur rows -- and reads 6 blur rows instead of 10 (front8.hip, dense_window).  The first dense
window of a stretch (after a sparse window, or at the start of a run) is the cold form, which carries nothing in.

What can go wrong is carried state that is stale or belongs to somebody else: across a run start, a frame, a sparse
window in between, a window that ends the run half way.  The cases are small frames built around those seams; every one
compares the fast path's own bit planes (hc_debug_tap) with the oracle's and the final maps with oracle.canny_r_batch,
bit for bit."""
import numpy as np
import pytest

from cudacam_amd import api, synth

from test_gpu_parity import _diff, _images

pytestmark = pytest.mark.gpu

# (dense mode, enter, leave): automatic at the library's thresholds; automatic, dense after any window with two candidates
ENTER_LEAVE = [(-1, 512, 384), (-1, 1, 0)]


def _check(oracle, frames, what, dense=-1, enter=None, leave=None, chunk=0, pipeline=0, half=None, low=10, high=40):
    frames = np.ascontiguousarray(frames)
    bgr = frames.ndim == 4
    n, h, w = frames.shape[:3]
    want_thr = [oracle.canny_r(f, low, high, stages=True)["thresh"] for f in frames]
    want = oracle.canny_r_batch(frames, low, high) if not bgr else [oracle.canny_r(f, low, high) for f in frames]
    with api.Context(w, h, 3 if bgr else 1, n) as ctx:
        ctx.set_thresholds(low, high)
        ctx.set_option(api.OPT_FRONT_DENSE, dense)
        if enter is not None:
            ctx.set_option(api.OPT_TEST_DENSE_ENTER, enter)
            ctx.set_option(api.OPT_TEST_DENSE_LEAVE, leave)
        if half is not None:
            ctx.set_option(api.OPT_FRONT_HALF, half)
        ctx.set_option(api.OPT_PIPELINE, pipeline)
        ctx.set_option(api.OPT_DEBUG_TAPS, 1)
        if chunk:
            ctx.set_tuning(chunk, 0)
        got = ctx.process(frames)
        if half is not None:   # hc_last_run_info: form 4 is the half-strip form of k_front8, 2 the plain one; the planner may decline a request
            assert ctx.last_run_info()[2] == (4 if half else 2), f"{what}: front form {ctx.last_run_info()[2]}"
        thr = ctx.debug_tap(api.TAP_THRESH, n)
        for f in range(n):
            _diff(thr[f], want_thr[f], f"{what}, frame {f}: bit planes")
            _diff(got[f], want[f], f"{what}, frame {f}: edges")


@pytest.mark.parametrize("h", [13, 14, 19, 20, 38])
def test_carry_short_runs_two_strips(oracle, h):
    """520 columns: a full strip and one with 24 live columns; a run of 3, 4 or 7 windows whose last one ends mid-window."""
    frames = np.stack([synth.noise(520, h, 100 + h), synth.noise(520, h, 200 + h)])
    _check(oracle, frames, f"520x{h} noise, every window dense", dense=1, half=0)
    _check(oracle, frames, f"520x{h} noise, enter 1 / leave 0", enter=1, leave=0, half=0)


def test_carry_cold_window_only(oracle):
    _check(oracle, synth.noise(64, 7, 3)[None], "64x7 noise, every window dense", dense=1)
    _check(oracle, synth.noise(64, 7, 3)[None], "64x7 noise, enter 1 / leave 0", enter=1, leave=0)


@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("chunk", [8, 12, 18])
def test_carry_stops_at_run_starts(oracle, chunk, pipeline):
    """Forced run lengths: warm windows meet run starts; nothing carried may cross a run or a frame.  The frames differ
    (noise, its mirror image, a strong step), so state leaking from one frame or run into the next changes the planes."""
    a = synth.noise(520, 61, 40 + chunk)
    frames = np.stack([a, a[::-1, ::-1].copy(), synth.steps(520, 61, 250, "diagonal")])
    _check(oracle, frames, f"runs of {chunk}, pipeline {pipeline}, every window dense", dense=1, chunk=chunk, pipeline=pipeline, half=0)
    _check(oracle, frames, f"runs of {chunk}, pipeline {pipeline}, enter 1 / leave 0", enter=1, leave=0, chunk=chunk, pipeline=pipeline, half=0)


def _bands(w, h, band, seed):
    """Rows alternate between bands of noise and flat bands: dense -> sparse -> dense within one run."""
    img = np.full((h, w), 90, np.uint8)
    nz = synth.noise(w, h, seed)
    for y0 in range(0, h, 2 * band):
        img[y0:y0 + band] = nz[y0:y0 + band]
    return img


@pytest.mark.parametrize("dense,enter,leave", ENTER_LEAVE, ids=["512_384", "1_0"])
@pytest.mark.parametrize("band", [6, 12, 18])
def test_carry_after_sparse_windows(oracle, band, dense, enter, leave):
    """The warm form follows a cold one that itself followed the queue path, in runs of the library's choice and in short ones.
    992 columns are two full strips: a window of 6 noise rows counts nearly all of its 744 half-lanes.  Any 12 rows hold a
    whole window, so at 512 / 384 the window after it is dense (cold) in the bands of 12 and 18 rows; 18 rows hold two,
    so the one after that counts more than 384 and is warm.  Bands of 6 rows reach 512 only where a window happens to
    coincide with one (the runs of 44 rows shift the windows against the bands); at 1 / 0 every band does."""
    frames = np.stack([_bands(992, 150, band, 7 * band), _bands(992, 150, band, 7 * band + 1)[::-1].copy()])
    _check(oracle, frames, f"bands of {band}, enter {enter} / leave {leave}", dense=dense, enter=enter, leave=leave)
    _check(oracle, frames, f"bands of {band}, enter {enter} / leave {leave}, runs of 44", dense=dense, enter=enter, leave=leave, chunk=44)


_SEAMS = ("step255_v", "step240_h", "step234_d", "noise_641x479", "noise_5x5", "one_px", "flat255_300x70", "noise_497x130", "natural_249x17")


@pytest.mark.parametrize("name,img", [(n, i) for n, i in _images() if n in _SEAMS], ids=[n for n, _ in _images() if n in _SEAMS])
def test_carry_wrap_bands_and_borders(oracle, name, img):
    """The u8 wrap bands of strong steps and the frame borders (zero padding of rows and columns), cold and warm windows."""
    _check(oracle, img[None], f"{name}, every window dense", dense=1)
    _check(oracle, img[None], f"{name}, enter 1 / leave 0", enter=1, leave=0)


@pytest.mark.parametrize("nb", [1, 5])
def test_carry_half_strip_form(oracle, nb):
    """240-column half-waves: the two halves of a wave belong to different strips and, with 5 frames of 3 units, to different frames."""
    frames = np.stack([synth.noise(640, 50, 60 + f) if f % 2 == 0 else _bands(640, 50, 12, 60 + f) for f in range(nb)])
    _check(oracle, frames, f"half-strip form, batch {nb}, every window dense", dense=1, half=1)
    _check(oracle, frames, f"half-strip form, batch {nb}, enter 1 / leave 0", enter=1, leave=0, half=1, chunk=20)


@pytest.mark.parametrize("pipeline", [0, 1])
def test_carry_fused_grey(oracle, pipeline):
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (2, 45, 520, 3), dtype=np.uint8)
    frames[1, 12:24] = 77
    _check(oracle, frames, f"BGR, pipeline {pipeline}, every window dense", dense=1, pipeline=pipeline)
    _check(oracle, frames, f"BGR, pipeline {pipeline}, enter 1 / leave 0", enter=1, leave=0, pipeline=pipeline, chunk=18)


@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("nb", [1, 5])
def test_carry_batches_default_thresholds(oracle, nb, pipeline):
    """The automatic mode as shipped: noise frames go dense after their first window and stay warm to the end of each run."""
    frames = np.stack([synth.noise(1000, 90, 80 + f) if f != 3 else synth.natural(1000, 90, 83) for f in range(nb)])
    _check(oracle, frames, f"batch {nb}, pipeline {pipeline}, automatic", pipeline=pipeline)
    _check(oracle, frames, f"batch {nb}, pipeline {pipeline}, automatic, 60/200", pipeline=pipeline, low=60, high=200)
