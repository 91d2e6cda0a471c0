"""Mode O beyond aperture 3 on the MI355X: HC_OPT_APERTURE 5 (cv::Canny(img, low, high, 5, L2)) and
hc_run_gradients_device (cv::Canny(dx, dy, edges, low, high, L2)), both k_front_o_ext, against the numpy restatement
(tests/canny_o_ext_ref.py, anchored to the oracle by tests/test_canny_o_ext_cpu.py)."""
import numpy as np
import pytest

from cudacam_amd import api, synth
import canny_o_ext_ref as X

pytestmark = pytest.mark.gpu


def _diff(a, b, what):
    if np.array_equal(a, b):
        return
    bad = np.argwhere(a != b)
    first = [(tuple(int(v) for v in p), int(a[tuple(p)]), int(b[tuple(p)])) for p in bad[:8]]
    raise AssertionError(f"{what}: {len(bad)} of {a.size} differ; first (pos, hip, ref): {first}")


def _rgb(w, h, seed):
    return np.stack([synth.natural(w, h, seed), synth.noise(w, h, seed + 1), synth.natural(w, h, seed + 2)[::-1].copy()], -1)


def _want5(frames, low, high, l2):
    return np.stack([X.canny_o(f, low, high, ksize=5, l2=l2) for f in frames])


def _ctx(w, h, ch, nb, aperture=5, l2=False, low=50, high=150):
    ctx = api.Context(w, h, ch, nb, api.MODE_O)
    ctx.set_thresholds(low, high)
    if aperture != 3:
        ctx.set_option(api.OPT_APERTURE, aperture)
    if l2:
        ctx.set_option(api.OPT_L2_GRADIENT, 1)
    return ctx


def _run_device5(ctx, frames, pad=0):
    """run_device on a pitched device copy of u8 frames (pitch = row bytes + pad)."""
    import torch
    n, h, w = frames.shape[:3]
    ch = 1 if frames.ndim == 3 else 3
    pitch = w * ch + pad
    buf = np.zeros((n, h, pitch), np.uint8)
    buf[:, :, :w * ch] = frames.reshape(n, h, w * ch)
    d_in = torch.from_numpy(buf).cuda()
    d_out = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.run_device(d_in.data_ptr(), pitch, pitch * h, d_out.data_ptr(), w, w * h, n)
    ctx.sync()
    return d_out.cpu().numpy()


def _run_grad(ctx, dx, dy, pad=0):
    """run_gradients_device on device int16 planes with a pitch of 2 * C * W + 2 * pad bytes."""
    import torch
    dx, dy = np.asarray(dx, np.int16), np.asarray(dy, np.int16)
    n, h, w = dx.shape[:3]
    ch = 1 if dx.ndim == 3 else 3
    ep = w * ch + pad
    bx = np.full((n, h, ep), 0x5A5A, np.int16)   # padding with junk: never read as gradients
    by = np.full((n, h, ep), -0x5A5B, np.int16)
    bx[:, :, :w * ch] = dx.reshape(n, h, w * ch)
    by[:, :, :w * ch] = dy.reshape(n, h, w * ch)
    tx, ty = torch.from_numpy(bx).cuda(), torch.from_numpy(by).cuda()
    d_out = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.run_gradients_device(tx.data_ptr(), ty.data_ptr(), 2 * ep, 2 * ep * h, d_out.data_ptr(), w, w * h, n)
    ctx.sync()
    return d_out.cpu().numpy()


IMAGES5 = [
    ("natural_640x480", lambda: synth.natural(640, 480, 1), 200, 600),
    ("noise_641x479", lambda: synth.noise(641, 479, 2), 1000, 3000),
    ("noise_low", lambda: synth.noise(333, 222, 5), 0, 400),
    ("flat255", lambda: synth.flat(300, 70, 255), 50, 150),
    ("step_v", lambda: synth.steps(260, 64, 255, "vertical"), 50, 150),
    ("step_d", lambda: synth.steps(250, 250, 120, "diagonal"), 50, 150),
    ("serpentine", lambda: synth.serpentine(500, 300, amp=30, seed_amp=200), 300, 900),
    ("natural_1080p", lambda: synth.natural(1920, 1080, 9), 200, 600),
    ("natural_4k_strip", lambda: synth.natural(3840, 100, 10), 100, 300),
    ("one_px", lambda: np.array([[200]], np.uint8), 50, 150),
    ("two", lambda: synth.noise(2, 2, 3), 10, 30),
    ("four", lambda: synth.noise(4, 4, 6), 100, 300),
    ("five", lambda: synth.noise(5, 5, 4), 100, 300),
]


@pytest.mark.parametrize("l2", [False, True], ids=["L1", "L2"])
@pytest.mark.parametrize("name,make,low,high", IMAGES5, ids=[m[0] for m in IMAGES5])
def test_aperture5_mono(name, make, low, high, l2):
    img = make()
    h, w = img.shape
    want = _want5([img], low, high, l2)
    with _ctx(w, h, 1, 1, l2=l2, low=low, high=high) as ctx:
        _diff(ctx.process(img), want, f"aperture 5 {name} process")
        assert ctx.last_run_info()[2] == 6
        _diff(_run_device5(ctx, img[None], pad=0), want, f"aperture 5 {name} run_device tight")
        _diff(_run_device5(ctx, img[None], pad=9), want, f"aperture 5 {name} run_device pitched")


@pytest.mark.parametrize("l2", [False, True], ids=["L1", "L2"])
@pytest.mark.parametrize("w,h", [(101, 77), (1, 1), (2, 2), (5, 5), (640, 480)])
def test_aperture5_rgb(w, h, l2):
    img = _rgb(w, h, 20 + w)
    want = _want5([img], 300, 900, l2)
    with _ctx(w, h, 3, 1, l2=l2, low=300, high=900) as ctx:
        _diff(ctx.process(img), want, "aperture 5 rgb process")
        _diff(_run_device5(ctx, img[None], pad=5), want, "aperture 5 rgb run_device")


def test_aperture5_batch_and_4k():
    frames = np.stack([synth.natural(700, 300, 60 + k) if k % 2 else synth.noise(700, 300, 60 + k) for k in range(8)])
    with _ctx(700, 300, 1, 8, low=400, high=1200) as ctx:
        _diff(ctx.process(frames), _want5(frames, 400, 1200, False), "aperture 5 batch of 8")
    img = _rgb(3840, 2160, 5)
    with _ctx(3840, 2160, 3, 1, low=300, high=900) as ctx:
        _diff(ctx.process(img), _want5([img], 300, 900, False), "aperture 5 3840x2160x3")


def _rand_grad(shape, seed):
    rng = np.random.default_rng(seed)
    dx = rng.integers(-32768, 32768, size=shape, dtype=np.int64)
    dy = rng.integers(-32768, 32768, size=shape, dtype=np.int64)
    flat = dx.reshape(-1)
    k = flat.size
    flat[rng.integers(0, k, size=max(1, k // 10))] = -32768            # the extremes
    dy.reshape(-1)[rng.integers(0, k, size=max(1, k // 20))] = -32768
    big = rng.integers(0, k, size=max(1, k // 5))                      # the tg67x wrap region
    flat[big] = rng.integers(27146, 32769, size=big.size) * rng.choice([-1, 1], size=big.size)
    both = rng.integers(0, k, size=max(1, k // 50))                    # L2 magnitude wraps to INT_MIN
    flat[both] = -32768
    dy.reshape(-1)[both] = -32768
    return np.clip(dx, -32768, 32767).astype(np.int16), dy.astype(np.int16)


@pytest.mark.parametrize("l2", [False, True], ids=["L1", "L2"])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h,pad", [(333, 201, 0), (331, 97, 0), (257, 60, 7), (1, 1, 0), (3, 2, 1), (1920, 64, 0)])
def test_gradients_full_range(w, h, pad, ch, l2):
    shape = (2, h, w) if ch == 1 else (2, h, w, 3)
    dx, dy = _rand_grad(shape, w * 7 + h + ch)
    for low, high in ((20000, 30000), (0, 32767), (32767, 30000)):
        want = np.stack([X.canny_o_from_gradients(dx[k], dy[k], low, high, l2) for k in range(2)])
        with _ctx(w, h, ch, 2, aperture=3, l2=l2, low=low, high=high) as ctx:
            _diff(_run_grad(ctx, dx, dy, pad), want, f"gradients {w}x{h}x{ch} pad {pad} L2 {l2} thr {low},{high}")
            assert ctx.last_run_info()[2] == 7


@pytest.mark.parametrize("l2", [False, True], ids=["L1", "L2"])
@pytest.mark.parametrize("ch", [1, 3])
def test_gradients_of_natural_images_and_cross_paths(ch, l2):
    """The gradient entry fed sobel_o(img, k) equals hc_run at aperture k (3 and 5)."""
    w, h = 517, 203   # odd width: tight int16 rows have a pitch = 2 mod 4
    imgs = np.stack([synth.natural(w, h, 30 + k) if ch == 1 else _rgb(w, h, 30 + k) for k in range(3)])
    for k, (low, high) in ((3, (50, 150)), (5, (300, 900))):
        g = [X.sobel_o(f, k) for f in imgs]
        dx = np.stack([a for a, _ in g]).astype(np.int16)
        dy = np.stack([b for _, b in g]).astype(np.int16)
        want = np.stack([X.canny_o_from_gradients(a, b, low, high, l2) for a, b in g])
        with _ctx(w, h, ch, 3, aperture=k, l2=l2, low=low, high=high) as ctx:
            direct = ctx.process(imgs)
            _diff(direct, want, f"hc_run aperture {k}")
            _diff(_run_grad(ctx, dx, dy, 0), direct, f"gradient entry vs hc_run, aperture {k}")
            _diff(ctx.process_gradients(dx, dy), direct, f"process_gradients, aperture {k}")


def test_gradients_host_continuation():
    """A weak vertical line of 2300 rows with a strong head, one hysteresis launch queued: the flood needs one launch per
    row tile, so the host-side continuation (hc_hysteresis_totals) must finish it."""
    w, h = 1000, 2300
    dx = np.zeros((1, h, w), np.int16)
    dy = np.zeros((1, h, w), np.int16)
    dx[0, :, 120] = 100          # candidate (50 < m <= 150), horizontal direction, neighbours 0
    dx[0, :4, 120] = 1000        # the strong head
    want = X.canny_o_from_gradients(dx[0], dy[0], 50, 150)[None]
    assert want[0, :, 120].all()
    with _ctx(w, h, 1, 1, aperture=3) as ctx:
        ctx.set_tuning(0, 1)
        ctx.hysteresis_totals(reset=True)
        _diff(_run_grad(ctx, dx, dy), want, "line of given gradients")
        assert ctx.hysteresis_totals()[1] >= 1, "the continuation did not run"


@pytest.mark.parametrize("w", [640, 641])
@pytest.mark.parametrize("caller_stream", [False, True])
def test_pipelined(w, caller_stream):
    import torch
    h = 200
    frames = [np.stack([synth.natural(w, h, 80 + 3 * r + f) for f in range(2)]) for r in range(3)]
    want5 = [_want5(b, 300, 900, False) for b in frames]
    grads = [[X.sobel_o(f, 3) for f in b] for b in frames]
    wantg = [np.stack([X.canny_o_from_gradients(a, c, 50, 150) for a, c in g]) for g in grads]
    d_in = [torch.from_numpy(b).cuda() for b in frames]
    d_gx = [torch.from_numpy(np.stack([a for a, _ in g]).astype(np.int16)).cuda() for g in grads]
    d_gy = [torch.from_numpy(np.stack([c for _, c in g]).astype(np.int16)).cuda() for g in grads]
    outs = [torch.zeros((2, h, w), dtype=torch.uint8, device="cuda") for _ in range(3)]
    outg = [torch.zeros((2, h, w), dtype=torch.uint8, device="cuda") for _ in range(3)]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _ctx(w, h, 1, 2, low=300, high=900) as ctx:
        ctx.set_option(api.OPT_PIPELINE, 1)
        if caller_stream:
            ctx.set_stream(s.cuda_stream)
        for r in range(3):
            ctx.run_device(d_in[r].data_ptr(), w, w * h, outs[r].data_ptr(), w, w * h, 2)
        ctx.sync()
        for r in range(3):
            _diff(outs[r].cpu().numpy(), want5[r], f"pipelined aperture 5 run {r}")
        ctx.set_thresholds(50, 150)
        for r in range(3):
            ctx.run_gradients_device(d_gx[r].data_ptr(), d_gy[r].data_ptr(), 2 * w, 2 * w * h, outg[r].data_ptr(), w, w * h, 2)
        ctx.sync()
        for r in range(3):
            _diff(outg[r].cpu().numpy(), wantg[r], f"pipelined gradients run {r}")


def test_thresh_tap_and_profiling():
    w, h = 301, 123
    img = _rgb(w, h, 44)
    with _ctx(w, h, 3, 1, low=300, high=900) as ctx:
        ctx.set_option(api.OPT_DEBUG_TAPS, 1)
        ctx.enable_profiling(1)
        _, pre = X.canny_o(img, 300, 900, ksize=5, premap=True)
        ctx.process(img)
        _diff(ctx.debug_tap(api.TAP_THRESH)[0], pre, "HC_TAP_THRESH aperture 5")
        assert ctx.last_run_info()[2] == 6
        t = [ctx.stage_time_ms(s) for s in range(6)]
        assert t[api.CannyStage.GAUSSIAN] < 0 and all(t[s] > 0 for s in (2, 3, 4, 5)), t
        dx, dy = X.sobel_o(img, 5)
        ctx.set_thresholds(300, 900)
        _, preg = X.canny_o_from_gradients(dx, dy, 300, 900, premap=True)
        _run_grad(ctx, dx[None], dy[None])
        _diff(ctx.debug_tap(api.TAP_THRESH)[0], preg, "HC_TAP_THRESH gradients")
        assert ctx.last_run_info()[2] == 7
        t = [ctx.stage_time_ms(s) for s in range(6)]
        assert t[api.CannyStage.GRADIENT] == -1 and all(t[s] > 0 for s in (3, 4, 5)), t


def test_errors():
    import torch
    with api.Context(64, 32, 1, 2, api.MODE_R) as ctx:
        with pytest.raises(api.HipCannyError):
            ctx.set_option(api.OPT_APERTURE, 5)
        with pytest.raises(api.HipCannyError):
            ctx.run_gradients_device(1 << 20, 1 << 21, 128, 128 * 32, 1 << 22, 64, 64 * 32, 1)
    with api.Context(64, 32, 1, 2, api.MODE_O) as ctx:
        for bad in (7, 4, 1, 0, -1):
            with pytest.raises(api.HipCannyError) as ei:
                ctx.set_option(api.OPT_APERTURE, bad)
            if bad == 7:
                assert "not offered" in str(ei.value)
        gx = torch.zeros((2, 32, 66), dtype=torch.int16, device="cuda")
        out = torch.zeros((2, 32, 64), dtype=torch.uint8, device="cuda")
        px, py, po = gx.data_ptr(), gx.data_ptr(), out.data_ptr()
        for args in ((px + 1, py, 132, 132 * 32), (px, py + 1, 132, 132 * 32), (px, py, 131, 131 * 32), (px, py, 132, 132 * 32 + 1),
                     (px, py, 126, 126 * 32), (0, py, 132, 132 * 32)):
            with pytest.raises(api.HipCannyError):
                ctx.run_gradients_device(*args, po, 64, 64 * 32, 1)
        for n in (0, 3):
            with pytest.raises(api.HipCannyError):
                ctx.run_gradients_device(px, py, 132, 132 * 32, po, 64, 64 * 32, n)
        ctx.run_gradients_device(px, py, 132, 132 * 32, po, 64, 64 * 32, 2)   # and the valid call runs
        ctx.sync()
        assert not out.any()


def test_fuzz():
    """~300 seeded cases: sizes up to 700 x 300, 1 / 3 channels, L1 / L2, thresholds, aperture 5 and the gradient entry, rows
    per work item (hc_set_tuning) from 1 to more than the frame."""
    rng = np.random.default_rng(20261016)
    bad = []
    for case in range(300):
        w, h = int(rng.integers(1, 701)), int(rng.integers(1, 301))
        if case % 3 == 0:
            w, h = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        ch = int(rng.choice([1, 3]))
        l2 = bool(rng.integers(0, 2))
        grad = bool(rng.integers(0, 2))
        seed = int(rng.integers(0, 1 << 30))
        kind = int(rng.integers(0, 3))
        mk = (lambda s: synth.natural(w, h, s)) if kind == 0 else (lambda s: synth.noise(w, h, s)) if kind == 1 else (
            lambda s: synth.serpentine(max(w, 1), max(h, 1), amp=20, seed_amp=200) if w > 40 and h > 40 else synth.natural(w, h, s))
        img = mk(seed) if ch == 1 else np.stack([mk(seed), mk(seed + 1), mk(seed + 2)], -1)
        # rows per work item: from a second generator seeded from the case seed (the main stream, and with it the sizes and
        # contents of the cases, stays as it was)
        chunk = int(np.random.default_rng([seed, 0xC4A2]).choice([0, 0, 1, 2, 3, 5, 7, 8, 13, 17, 50, 300]))
        if grad:
            if rng.integers(0, 2):
                dx, dy = _rand_grad((1, h, w) if ch == 1 else (1, h, w, 3), seed)
            else:
                a, b = X.sobel_o(img, int(rng.choice([3, 5])))
                dx, dy = a[None].astype(np.int16), b[None].astype(np.int16)
            low, high = (int(v) for v in rng.integers(0, 32768, size=2))
            want = X.canny_o_from_gradients(dx[0], dy[0], low, high, l2)[None]
            with _ctx(w, h, ch, 1, aperture=3, l2=l2, low=low, high=high) as ctx:
                ctx.set_tuning(chunk, 0)
                got = _run_grad(ctx, dx, dy, int(rng.integers(0, 3)))
        else:
            low, high = (int(v) for v in rng.integers(0, 3000, size=2))
            want = _want5([img], low, high, l2)
            with _ctx(w, h, ch, 1, l2=l2, low=low, high=high) as ctx:
                ctx.set_tuning(chunk, 0)
                got = ctx.process(img) if rng.integers(0, 2) else _run_device5(ctx, img[None], int(rng.integers(0, 5)))
        if not np.array_equal(got, want):
            bad.append((case, w, h, ch, l2, grad, chunk, int((got != want).sum())))
    assert not bad, f"{len(bad)} of 300 cases differ: {bad[:10]}"
