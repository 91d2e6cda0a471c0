"""hc_canny_device on the MI355X: cv::Canny(img, edges, low, high, apertureSize, L2gradient) in one call, with the fused
aperture-7 and Scharr sources of k_front_o_ext (front forms 8 / 9).  Every comparison is bit-exact.  The reference is
tests/deriv_ref.py's sobel16 followed by tests/canny_o_ext_ref.py's canny_o_from_gradients with thresholds low / s,
high / s (s = 16 at aperture 7, 1 elsewhere): numpy restatements that share nothing with the kernels.

Shapes are the smallest at which the kernel takes another path: widths of one pixel, a lane group +- 1 and the 248-column
strip +- 1, once and twice; heights 1 .. 10; work items of 1 .. 16 rows on a 29 x 253 frame (every residue of the ring
periods 7, 6, 3 and 2, last items of one row)."""
import numpy as np
import pytest
from scipy import ndimage

from cudacam_amd import api
import canny_o_ext_ref as X
import deriv_ref as D
import view_arena as VA

pytestmark = pytest.mark.gpu

FORM = {7: api.FORM_O_APERTURE7, -1: api.FORM_O_SCHARR}
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 244, 247, 248, 249, 252, 253, 496, 497)
HEIGHTS = tuple(range(1, 11))
CONTENTS = ("random", "smooth", "zeros", "full", "checker")


def _scale(ap):
    return 16.0 if ap == 7 else 1.0


def _plane(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "smooth":   # Gaussian-smoothed random, stretched to 0..255
        g = ndimage.gaussian_filter(rng.random((h, w)), 2.0, mode="nearest")
        span = float(g.max() - g.min())
        return np.round((g - g.min()) / span * 255.0).astype(np.uint8) if span > 0 else np.full((h, w), 128, np.uint8)
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    if kind == "full":    # replicate border: no edge anywhere
        return np.full((h, w), 255, np.uint8)
    if kind == "checker":  # 1-px checkerboard: the largest sums (S = +-163200 at aperture 7)
        return (((np.arange(h)[:, None] + np.arange(w)[None, :] + seed) & 1) * 255).astype(np.uint8)
    raise ValueError(kind)


def _image(kind, w, h, ch, seed):
    if ch == 1:
        return _plane(kind, w, h, seed)
    return np.stack([_plane(kind, w, h, seed + 101 * c) for c in range(3)], -1)


def _selected_magnitude(dx, dy, l2):
    dx, dy = np.asarray(dx, np.int64), np.asarray(dy, np.int64)
    m = dx * dx + dy * dy if l2 else np.abs(dx) + np.abs(dy)
    return m if m.ndim == 2 else m.max(axis=-1)


def _quantile_thresholds(dx, dy, ap, l2):
    """low / high in cv::Canny's units from the 60th and 85th percentile of the reference's own selected magnitude."""
    m = _selected_magnitude(dx, dy, l2)
    lo, hi = np.percentile(m, 60), np.percentile(m, 85)
    if l2:   # the call squares its thresholds
        lo, hi = np.sqrt(lo), np.sqrt(hi)
    return float(lo) * _scale(ap), float(hi) * _scale(ap)


def _want(img, low, high, ap, l2, premap=False, grads=None):
    dx, dy = grads if grads is not None else D.sobel16(img, ap)
    return X.canny_o_from_gradients(dx, dy, low / _scale(ap), high / _scale(ap), l2, premap)


def _diff(got, want, what):
    if np.array_equal(got, want):
        return None
    bad = np.argwhere(got != want)
    first = [(tuple(int(v) for v in p), int(got[tuple(p)]), int(want[tuple(p)])) for p in bad[:6]]
    return f"{what}: {len(bad)} of {want.size} differ; first (pos, hip, ref): {first}"


def _check(got, want, what):
    msg = _diff(got, want, what)
    assert msg is None, msg


def _ctx(w, h, ch, nb=1):
    return api.Context(w, h, ch, nb, api.MODE_O)


# ---------------------------------------------------------------------------------------------------------------------
# shape and content sweep
# ---------------------------------------------------------------------------------------------------------------------
_REF_CACHE = {}


def _sweep_reference(ap, ch, w, h):
    """Per content: image, its derivatives (computed once, shared by the L1 and L2 tests, never changed)."""
    key = (ap, ch, w, h)
    if key not in _REF_CACHE:
        out = []
        for k, kind in enumerate(CONTENTS):
            img = _image(kind, w, h, ch, 1000 * w + 10 * h + k)
            out.append((kind, img, D.sobel16(img, ap)))
        _REF_CACHE[key] = out
    return _REF_CACHE[key]


@pytest.mark.parametrize("l2", [False, True], ids=["L1", "L2"])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("ap", [7, -1], ids=["aperture7", "scharr"])
def test_shape_and_content_sweep(ap, ch, l2):
    bad, cases = [], 0
    for w in WIDTHS:
        for h in HEIGHTS:
            with _ctx(w, h, ch) as ctx:
                for kind, img, grads in _sweep_reference(ap, ch, w, h):
                    low, high = _quantile_thresholds(*grads, ap, l2)
                    got = ctx.canny(img, low, high, ap, l2)[0]
                    cases += 1
                    msg = _diff(got, _want(img, low, high, ap, l2, grads=grads), f"{w}x{h}x{ch} {kind} thr ({low:.3f}, {high:.3f})")
                    if msg:
                        bad.append(msg)
                assert ctx.last_run_info()[2] == FORM[ap]
    assert cases == len(WIDTHS) * len(HEIGHTS) * len(CONTENTS)
    assert not bad, f"{len(bad)} of {cases} cases differ: {bad[:5]}"


@pytest.mark.parametrize("ch", [1, 3])
def test_l2_thresholds_that_are_no_multiples_of_16(ch):
    """Aperture 7 with L2gradient divides, squares and only then floors: (1000, 3000) / 16 = (62.5, 187.5) -> 3906, 35156,
    which no pair of integer context thresholds expresses (62^2 = 3844, 63^2 = 3969)."""
    assert X.thresholds(1000 / 16.0, 3000 / 16.0, True) == (3906, 35156)
    w, h = 253, 29
    for kind in ("random", "smooth"):
        img = _image(kind, w, h, ch, 77)
        for low, high in ((1000, 3000), (1000.5, 2999.75), (3000, 1000)):
            with _ctx(w, h, ch) as ctx:
                _check(ctx.canny(img, low, high, 7, True)[0], _want(img, low, high, 7, True), f"aperture 7 L2 {kind} ({low}, {high})")
                _check(ctx.canny(img, low, high, -1, True)[0], _want(img, low, high, -1, True), f"Scharr L2 {kind} ({low}, {high})")


# ---------------------------------------------------------------------------------------------------------------------
# the flood is exercised: candidates that are promoted, candidates that are dropped
# ---------------------------------------------------------------------------------------------------------------------
def _flood_stats(img, low, high, ap, l2=False):
    out, pre = _want(img, low, high, ap, l2, premap=True)
    cand = pre == 128
    return float(cand.mean()), int((cand & (out == 255)).sum()), int((cand & (out == 0)).sum())


@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("ap", [7, -1], ids=["aperture7", "scharr"])
def test_flood_promotes_and_drops(ap, kind):
    """29 x 253: for at least one threshold pair of the group the reference's pre-flood map has >= 1 % candidate-only pixels
    and its flood both promotes and drops some of them -- asserted on the reference, then every pair is compared."""
    w, h = 253, 29
    img = _image(kind, w, h, 1, 5)
    grads = D.sobel16(img, ap)
    pairs = [_quantile_thresholds(*grads, ap, False)]
    if ap == -1:
        pairs.append((1200.0, 2600.0) if kind == "random" else (300.0, 900.0))
    else:
        pairs += [(1000.0, 3000.0), (4000.0, 9000.0)]
    stats = [_flood_stats(img, lo, hi, ap) for lo, hi in pairs]
    print(f"aperture {ap} {kind}: (low, high) -> (candidate share, promoted, dropped): {list(zip(pairs, stats))}")
    assert any(share >= 0.01 and promoted > 0 and dropped > 0 for share, promoted, dropped in stats), (pairs, stats)
    with _ctx(w, h, 1) as ctx:
        ctx.set_option(api.OPT_DEBUG_TAPS, 1)
        for lo, hi in pairs:
            want, pre = _want(img, lo, hi, ap, False, premap=True, grads=grads)
            _check(ctx.canny(img, lo, hi, ap, False)[0], want, f"aperture {ap} {kind} ({lo}, {hi})")
            _check(ctx.debug_tap(api.TAP_THRESH)[0], pre, f"aperture {ap} {kind} ({lo}, {hi}) pre-flood map")


# ---------------------------------------------------------------------------------------------------------------------
# work-item seams
# ---------------------------------------------------------------------------------------------------------------------
SEAM_W, SEAM_H = 253, 29
SEAM_ROWS = tuple(range(1, 17)) + (SEAM_H, SEAM_H + 5)


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("ap", [7, -1], ids=["aperture7", "scharr"])
def test_work_item_seams(ap, ch):
    """hc_set_tuning's rows per work item 1 .. 16, H and H + 5: plain runs with the THRESH tap against the reference's
    pre-flood map, pipelined runs two in flight on rotating outputs."""
    import torch
    w, h = SEAM_W, SEAM_H
    imgs = [_image("random", w, h, ch, 31), _image("smooth", w, h, ch, 32)]
    thr = [_quantile_thresholds(*D.sobel16(f, ap), ap, False) for f in imgs]
    wants = [_want(f, lo, hi, ap, False, premap=True) for f, (lo, hi) in zip(imgs, thr)]
    d_in = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in imgs]
    outs = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    row = w * ch
    bad = []
    with _ctx(w, h, ch) as ctx:
        for rows in SEAM_ROWS:
            ctx.set_option(api.OPT_PIPELINE, 0)
            ctx.set_option(api.OPT_DEBUG_TAPS, 1)
            ctx.set_tuning(rows, 0)
            for k in range(2):
                outs[0].fill_(7)
                torch.cuda.synchronize()
                ctx.canny_device(d_in[k].data_ptr(), row, row * h, outs[0].data_ptr(), w, w * h, 1, thr[k][0], thr[k][1], ap, False)
                ctx.sync()
                assert ctx.last_run_info() == (w % 4 != 0, w % 4 != 0, FORM[ap])   # tight rows of 253 columns: staged on both sides
                bad.append(_diff(ctx.debug_tap(api.TAP_THRESH)[0], wants[k][1], f"rows {rows} plain frame {k} pre-flood map"))
                bad.append(_diff(outs[0].cpu().numpy(), wants[k][0], f"rows {rows} plain frame {k}"))
            ctx.set_option(api.OPT_DEBUG_TAPS, 0)
            ctx.set_option(api.OPT_PIPELINE, 1)
            for o in outs:
                o.fill_(7)
            torch.cuda.synchronize()
            for r in range(4):   # in flight together, each into an output of its own
                k = r % 2
                ctx.canny_device(d_in[k].data_ptr(), row, row * h, outs[r].data_ptr(), w, w * h, 1, thr[k][0], thr[k][1], ap, False)
            ctx.sync()
            for r in range(4):
                bad.append(_diff(outs[r].cpu().numpy(), wants[r % 2][0], f"rows {rows} pipelined run {r}"))
    bad = [b for b in bad if b]
    assert not bad, f"{len(bad)} differ: {bad[:5]}"


# ---------------------------------------------------------------------------------------------------------------------
# cross-path identities on the device
# ---------------------------------------------------------------------------------------------------------------------
def _batch(w, h, ch, n, seed):
    return np.stack([_image("smooth" if k % 2 else "random", w, h, ch, seed + k) for k in range(n)])


@pytest.mark.parametrize("l2", [False, True], ids=["L1", "L2"])
@pytest.mark.parametrize("ch", [1, 3])
def test_apertures_3_and_5_are_hc_run_device(ch, l2):
    """canny(..., 3 | 5) gives the bytes of hc_run with HC_OPT_APERTURE 3 | 5 and the same integer thresholds, and the same form."""
    w, h, n = 501, 67, 3
    frames = _batch(w, h, ch, n, 40)
    for ap, (low, high) in ((3, (120, 360)), (5, (1500, 4000))):
        with _ctx(w, h, ch, n) as ctx:
            ctx.set_thresholds(low, high)
            ctx.set_option(api.OPT_L2_GRADIENT, int(l2))
            if ap == 5:
                ctx.set_option(api.OPT_APERTURE, 5)
            via_options = ctx.process(frames)
            form = ctx.last_run_info()[2]
            assert form == (6 if ap == 5 else 3 if ch == 1 else -1)
            assert via_options.any()
        with _ctx(w, h, ch, n) as ctx:   # a context whose own thresholds and options say something else
            ctx.set_thresholds(1, 2)
            ctx.set_option(api.OPT_L2_GRADIENT, int(not l2))
            _check(ctx.canny(frames, low, high, ap, l2), via_options, f"aperture {ap} L2 {l2}: canny against the option path")
            assert ctx.last_run_info()[2] == form
            if not l2:   # (floored after squaring: fractions only vanish from L1 thresholds)
                _check(ctx.canny(frames, high + 0.75, low + 0.25, ap, l2), via_options, f"aperture {ap}: swapped, fractional thresholds")
            _check(ctx.canny(frames, high, low, ap, l2), via_options, f"aperture {ap}: swapped thresholds")


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("ap", [7, -1], ids=["aperture7", "scharr"])
def test_fused_equals_the_chain(ap, ch):
    """canny(..., 7 | -1, L1) gives the bytes of process_aperture(7 | -1) -- k_deriv16, then the gradient entry -- with the
    context thresholds floor(low / s), floor(high / s)."""
    w, h, n = 501, 67, 3
    frames = _batch(w, h, ch, n, 50)
    low, high = (1000.0, 2777.0) if ap == 7 else (700.0, 2000.0)
    with _ctx(w, h, ch, n) as ctx:
        ctx.set_thresholds(int(low // _scale(ap)), int(high // _scale(ap)))
        chain = ctx.process_aperture(frames, ap)
        assert ctx.last_run_info()[2] == 7 and chain.any()
        _check(ctx.canny(frames, low, high, ap, False), chain, f"aperture {ap}: fused against the chain")
        assert ctx.last_run_info()[2] == FORM[ap]


# ---------------------------------------------------------------------------------------------------------------------
# state
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3])
def test_the_call_leaves_the_context_as_it_was(ch):
    w, h = 322, 41
    img = _image("smooth", w, h, ch, 60)
    want5 = X.canny_o(img, 300, 900, ksize=5, l2=False)
    with _ctx(w, h, ch) as ctx:
        ctx.set_thresholds(300, 900)
        ctx.set_option(api.OPT_APERTURE, 5)
        ctx.enable_profiling(1)
        for ap, l2, form in ((7, True, 8), (-1, False, 9), (5, True, 6), (3, True, 3 if ch == 1 else -1)):
            low, high = 160.0 * _scale(ap), 480.5 * _scale(ap)
            got = ctx.canny(img, low, high, ap, l2)[0]
            assert ctx.last_run_info()[2] == form
            t = [ctx.stage_time_ms(s) for s in range(6)]
            assert t[api.CannyStage.GAUSSIAN] == -1 and all(t[s] > 0 for s in (2, 3, 4, 5)), (ap, t)
            if ap in FORM:
                _check(got, _want(img, low, high, ap, l2), f"aperture {ap}")
            assert ctx.get_thresholds() == (300, 900)
            _check(ctx.process(img)[0], want5, f"HC_OPT_APERTURE 5 run after canny(aperture {ap})")   # L1: HC_OPT_L2_GRADIENT is still 0
            assert ctx.last_run_info()[2] == 6


# ---------------------------------------------------------------------------------------------------------------------
# views
# ---------------------------------------------------------------------------------------------------------------------
def _lead(pitch):
    return VA.round_up(pitch + 64, 512)


def _view_family(fam, w, h, ch):
    """((in pitch, frame stride, offset, fill), (out pitch, frame stride, offset))"""
    rb, w4 = w * ch, VA.round_up(w, 4)
    if fam == "tight":     # rows without whole 4-pixel groups when w % 4: staged
        return (rb, rb * h, 0, "random"), (w, w * h, 0)
    if fam == "pitched":   # everything a multiple of 4, nothing of 8: in place
        p, q = w4 * ch + 4, w4 + 4
        return (p, p * h + 20, 4, "ff"), (q, q * h + 20, 12)
    if fam == "roi":       # a rectangle of a parent image on both sides, in place
        p, q = VA.round_up((w + 27) * ch, 4), VA.round_up(w + 53, 4)
        return (p, p * (h + 7), 3 * p + 4 * ch, "parent"), (q, q * (h + 5), 2 * q + 36)
    if fam == "odd":       # odd pitch and pointer on both sides: staged
        p, q = w4 * ch + 1, w4 + 1
        return (p, p * h + 3, 1, "random"), (q, q * h + 1, 3)
    if fam == "odd_in":    # pitch = 2 mod 4 on the input only
        p = w4 * ch + 2
        return (p, p * h, 2, "ff"), (w4, w4 * h, 0)
    raise ValueError(fam)


@pytest.mark.parametrize("fam", ["tight", "pitched", "roi", "odd", "odd_in"])
@pytest.mark.parametrize("w,h,ch", [(253, 9, 1), (250, 5, 3), (8, 3, 3), (497, 4, 1)])
@pytest.mark.parametrize("ap", [7, -1], ids=["aperture7", "scharr"])
def test_views(ap, w, h, ch, fam):
    """Guarded arenas on both sides: nothing outside [row, row + width) of the output rows is written, the input is
    unchanged, the maps are exact; staging as hc_last_run_info promises for an aperture-5 run; plain and pipelined."""
    import torch
    n = 2
    (ip, ifs, ioff, fill), (op, ofs, ooff) = _view_family(fam, w, h, ch)
    seq = [np.stack([_image("random" if (f + r) % 2 else "smooth", w, h, ch, 7 * r + f + w) for f in range(n)]) for r in range(3)]
    thr = _quantile_thresholds(*D.sobel16(seq[0][0], ap), ap, False)
    want = [np.stack([_want(f, thr[0], thr[1], ap, False) for f in fr]) for fr in seq]
    exp_in = (ioff | ip | ifs) % 4 != 0 or ip < VA.round_up(w, 4) * ch
    exp_out = (ooff | op | ofs) % 4 != 0
    arenas = [VA.make_input(fr, ip, ifs, ioff, fill, lead=_lead(ip), seed=r + w)[0] for r, fr in enumerate(seq)]
    d_in = [torch.from_numpy(a).cuda() for a in arenas]
    in_off = _lead(ip) + ioff
    before = [VA.make_output(n, h, w, op, ofs, ooff, lead=_lead(op), seed=w + j) for j in range(2)]
    go = before[0][1]
    with _ctx(w, h, ch, n) as ctx:
        for piped in (0, 1):
            ctx.set_option(api.OPT_PIPELINE, piped)
            d_out = [torch.from_numpy(b[0]).cuda() for b in before]
            torch.cuda.synchronize()
            for r in ((0, 1, 2) if piped else (2,)):
                ctx.canny_device(d_in[r].data_ptr() + in_off, ip, ifs, d_out[r % 2].data_ptr() + go.offset, op, ofs, n, thr[0], thr[1], ap, False)
            ctx.sync()
            what = f"aperture {ap} {w}x{h}x{ch} {fam} {'pipelined' if piped else 'plain'}"
            assert ctx.last_run_info() == (exp_in, exp_out, FORM[ap]), f"{what}: {ctx.last_run_info()}"
            VA.check_output(d_out[0].cpu().numpy(), before[0][0], go, want[2], what + ", arena 0")
            if piped:
                VA.check_output(d_out[1].cpu().numpy(), before[1][0], go, want[1], what + ", arena 1")
            for r in range(3):
                assert np.array_equal(d_in[r].cpu().numpy(), arenas[r]), what + ": the input changed"


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    import torch
    w, h = 64, 32
    src = torch.full((2, h, w), 9, dtype=torch.uint8, device="cuda")
    out = torch.full((2, h, w), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pi, po = src.data_ptr(), out.data_ptr()
    with api.Context(w, h, 1, 2, api.MODE_R) as ctx:
        with pytest.raises(api.HipCannyError):
            ctx.canny_device(pi, w, w * h, po, w, w * h, 1, 50, 150, 7, False)
    with _ctx(w, h, 1, 2) as ctx:
        for ap in (0, 1, 4, 9, -3):
            with pytest.raises(api.HipCannyError):
                ctx.canny_device(pi, w, w * h, po, w, w * h, 1, 50, 150, ap, False)
        for low, high in ((float("nan"), 150), (50, float("nan")), (-1, 150), (50, -0.5), (float("inf"), 150)):
            for ap in (3, 7):
                with pytest.raises(api.HipCannyError):
                    ctx.canny_device(pi, w, w * h, po, w, w * h, 1, low, high, ap, False)
        for a, b in ((0, po), (pi, 0)):
            with pytest.raises(api.HipCannyError):
                ctx.canny_device(a, w, w * h, b, w, w * h, 1, 50, 150, 7, False)
        for n in (0, 3):
            with pytest.raises(api.HipCannyError):
                ctx.canny_device(pi, w, w * h, po, w, w * h, n, 50, 150, 7, False)
        with pytest.raises(api.HipCannyError):   # as hc_run_device: a pitch smaller than a row
            ctx.canny_device(pi, w - 1, w * h, po, w, w * h, 1, 50, 150, -1, False)
        assert (out == 7).all()
        for ap in (7, -1, 5, 3):                  # and the valid call runs: a flat frame has no edge
            ctx.canny_device(pi, w, w * h, po, w, w * h, 2, 50, 150, ap, True)
            ctx.sync()
            assert not out.any()
            out.fill_(7)
            torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# fuzz
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(4))
def test_fuzz(part):
    """~200 seeded cases in four parts: sizes up to 700 x 300, both new forms, 1 / 3 channels, L1 / L2, pitches and offsets,
    random rows per work item."""
    import torch
    rng = np.random.default_rng([20261018, part])
    bad = []
    for case in range(50):
        w, h = int(rng.integers(1, 701)), int(rng.integers(1, 301))
        if case % 3 == 0:
            w, h = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        ch, l2, ap = int(rng.choice([1, 3])), bool(rng.integers(0, 2)), int(rng.choice([7, -1]))
        kind = CONTENTS[int(rng.choice([0, 0, 1, 1, 4]))]
        img = _image(kind, w, h, ch, int(rng.integers(0, 1 << 30)))
        grads = D.sobel16(img, ap)
        low, high = _quantile_thresholds(*grads, ap, l2)
        if rng.integers(0, 3) == 0:
            low, high = float(rng.uniform(0, 2 * high + 1)), float(rng.uniform(0, 2 * high + 1))
        chunk = int(rng.choice([0, 0, 1, 2, 3, 5, 6, 7, 8, 13, 14, 17, 50, 300]))
        pad, off = int(rng.choice([0, 0, 1, 2, 4, 12])), int(rng.choice([0, 0, 1, 2, 4]))
        ip = w * ch + pad
        arena, a_off = VA.make_input(img[None], ip, None, off, "random", lead=_lead(ip), seed=case)
        d_in = torch.from_numpy(arena).cuda()
        d_out = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with _ctx(w, h, ch) as ctx:
            ctx.set_tuning(chunk, 0)
            ctx.canny_device(d_in.data_ptr() + a_off, ip, ip * h, d_out.data_ptr(), w, w * h, 1, low, high, ap, l2)
            ctx.sync()
            form = ctx.last_run_info()[2]
        msg = _diff(d_out.cpu().numpy(), _want(img, low, high, ap, l2, grads=grads), f"case {case}: {w}x{h}x{ch} aperture {ap} L2 {l2} {kind} rows {chunk} pad {pad} off {off}")
        if msg or form != FORM[ap]:
            bad.append(msg or f"case {case}: form {form}")
    assert not bad, f"{len(bad)} of 50 cases differ: {bad[:5]}"
