"""The numpy restatement of hc_pyr_down_device and hc_lk_flow_device as include/hipcanny.h states them: the device results must agree
with these bit for bit.  Window sums are exact int64, the float steps np.float32 scalars, one rounded operation each."""
import numpy as np

F = np.float32
TAPS = np.array([1, 4, 6, 4, 1], dtype=np.int64)
FLT_EPS = F(1.1920929e-7)


def reflect101(i, n):
    """BORDER_REFLECT_101 for -2 <= i <= n + 1, n >= 3: one reflection"""
    return -i if i < 0 else 2 * n - 2 - i if i >= n else i


def pyr_down(src):
    """cv::pyrDown of one u8 plane (H, W), H, W >= 3 -> ((H + 1) // 2, (W + 1) // 2)"""
    src = np.asarray(src)
    h, w = src.shape
    assert h >= 3 and w >= 3 and src.dtype == np.uint8
    dh, dw = (h + 1) // 2, (w + 1) // 2
    cols = np.array([[reflect101(2 * x + i, w) for i in range(-2, 3)] for x in range(dw)])
    rows = np.array([[reflect101(2 * y + j, h) for j in range(-2, 3)] for y in range(dh)])
    s = src.astype(np.int64)
    hs = (s[:, cols] * TAPS).sum(axis=2)           # (h, dw)
    vs = (hs[rows, :] * TAPS[None, :, None]).sum(axis=1)  # (dh, dw)
    return ((vs + 128) >> 8).astype(np.uint8)


def pyramid(img, levels):
    """[level 0 .. level L]: L <= levels, stopping at the last level whose sides are still at least 3 (as Context.optical_flow)"""
    out = [np.ascontiguousarray(img)]
    for _ in range(levels):
        h, w = out[-1].shape
        if (h + 1) // 2 < 3 or (w + 1) // 2 < 3:
            break
        out.append(pyr_down(out[-1]))
    return out


def _pix(img, x, y):
    h, w = img.shape
    return img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64)


def _scharr(img, x, y):
    """(Dx, Dy) at integer positions (arrays), every fetch clamped"""
    p = lambda dx, dy: _pix(img, x + dx, y + dy)
    dx = 3 * (p(1, -1) - p(-1, -1)) + 10 * (p(1, 0) - p(-1, 0)) + 3 * (p(1, 1) - p(-1, 1))
    dy = 3 * (p(-1, 1) - p(-1, -1)) + 10 * (p(0, 1) - p(0, -1)) + 3 * (p(1, 1) - p(1, -1))
    return dx, dy


def _out(q, win, w, h):
    ix, iy = np.floor(q[0]), np.floor(q[1])
    return not (ix >= F(-win) and ix < F(w) and iy >= F(-win) and iy < F(h))


def _weights(q):
    ix, iy = np.floor(q[0]), np.floor(q[1])
    a, b = F(q[0] - ix), F(q[1] - iy)
    t0, t1 = F(F(1) - a), F(F(1) - b)
    k = F(16384)
    w00 = int(np.rint(F(F(t0 * t1) * k)))
    w01 = int(np.rint(F(F(a * t1) * k)))
    w10 = int(np.rint(F(F(t0 * b) * k)))
    return int(ix), int(iy), (w00, w01, w10, 16384 - w00 - w01 - w10)


def _interp(fn, ix, iy, wts, ii, jj):
    x, y = ix + ii, iy + jj
    return wts[0] * fn(x, y) + wts[1] * fn(x + 1, y) + wts[2] * fn(x, y + 1) + wts[3] * fn(x + 1, y + 1)


def lk_point(prev, nxt, level, prev_pt, next_pt, win, max_iterations, epsilon, min_eig_threshold, use_initial):
    """One point of one level: (next_pt float32[2], status or None, err or None, info).  Points are level-0 units.  info says how the
    point went: the iterations run, whether the half-step stop fired, min_eig, why it was lost ("lost": None, or "start" -- the
    window around prev_pt is out of the frame --, "eigen", "left" -- an iteration's position is out --, "end" -- the final one is,
    at level 0), and the exact integer window sums where they were made (A11, A12, A22; B1, B2 of every iteration; err_sum)."""
    h, w = prev.shape
    s, S = F(2.0 ** -level), F(2.0 ** level)
    hw = F(F(win - 1) * F(0.5))
    prev_pt = np.asarray(prev_pt, dtype=F)
    start = np.asarray(next_pt if use_initial else prev_pt, dtype=F).copy()
    info = {"half_step": False, "iterations": 0, "lost": None, "B1": [], "B2": []}
    jj, ii = np.mgrid[0:win, 0:win]

    def finish(lost, v):
        if lost:
            out = start.copy()
        else:
            out = np.array([F(F(v[0] + hw) * S), F(F(v[1] + hw) * S)], dtype=F)
        if level != 0:
            return out, None, None, info
        ok = (not lost) and not _out(v, win, w, h)
        if not lost and not ok:
            info["lost"] = "end"
        err = F(0)
        if ok:
            ix, iy, wts = _weights(v)
            d = ((_interp(lambda x, y: _pix(nxt, x, y), ix, iy, wts, ii, jj) + 256) >> 9) - I
            info["err_sum"] = int(np.abs(d).sum())
            err = F(F(info["err_sum"]) / F(32 * win * win))
        return out, int(ok), err, info

    with np.errstate(all="ignore"):
        u = (F(F(prev_pt[0] * s) - hw), F(F(prev_pt[1] * s) - hw))
        if _out(u, win, w, h):
            info["lost"] = "start"
            return finish(True, None)
        ix, iy, wts = _weights(u)
        I = (_interp(lambda x, y: _pix(prev, x, y), ix, iy, wts, ii, jj) + 256) >> 9
        gx = (_interp(lambda x, y: _scharr(prev, x, y)[0], ix, iy, wts, ii, jj) + 8192) >> 14
        gy = (_interp(lambda x, y: _scharr(prev, x, y)[1], ix, iy, wts, ii, jj) + 8192) >> 14
        sc = F(2.0 ** -20)
        A11, A12, A22 = int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum())
        info.update(A11=A11, A12=A12, A22=A22)
        f11, f12, f22 = F(F(A11) * sc), F(F(A12) * sc), F(F(A22) * sc)
        D = F(F(f11 * f22) - F(f12 * f12))
        d = F(f11 - f22)
        m = F(F(f22 + f11) - np.sqrt(F(F(d * d) + F(F(4) * F(f12 * f12)))))
        min_eig = F(m / F(2 * win * win))
        info["min_eig"] = min_eig
        if min_eig < F(min_eig_threshold) or D < FLT_EPS:
            info["lost"] = "eigen"
            return finish(True, None)
        Dinv = F(F(1) / D)
        v = [F(F(start[0] * s) - hw), F(F(start[1] * s) - hw)]
        eps2 = F(float(epsilon) * float(epsilon))
        px = py = F(0)
        for k in range(max_iterations):
            if _out(v, win, w, h):
                info["lost"] = "left"
                return finish(True, None)
            info["iterations"] = k + 1
            ix, iy, wts = _weights(v)
            diff = ((_interp(lambda x, y: _pix(nxt, x, y), ix, iy, wts, ii, jj) + 256) >> 9) - I
            B1, B2 = int((diff * gx).sum()), int((diff * gy).sum())
            info["B1"].append(B1)
            info["B2"].append(B2)
            g1, g2 = F(F(B1) * sc), F(F(B2) * sc)
            ex = F(F(F(f12 * g2) - F(f22 * g1)) * Dinv)
            ey = F(F(F(f12 * g1) - F(f11 * g2)) * Dinv)
            v = [F(v[0] + ex), F(v[1] + ey)]
            if F(F(ex * ex) + F(ey * ey)) <= eps2:
                break
            if k > 0 and abs(F(ex + px)) < F(0.01) and abs(F(ey + py)) < F(0.01):
                v = [F(v[0] - F(ex * F(0.5))), F(v[1] - F(ey * F(0.5)))]
                info["half_step"] = True
                break
            px, py = ex, ey
        return finish(False, v)


def lk_level(prev, nxt, level, counts, prev_pts, next_pts, win, max_iterations, epsilon, min_eig_threshold, use_initial, status=None, err=None):
    """hc_lk_flow_device on host arrays: prev, nxt (n, h, w) u8; counts (n,); prev_pts, next_pts (n, capacity, 2) float32; status
    (n, capacity) u8 and err (n, capacity) float32 are updated at level 0 only.  Returns (next_pts, status, err) as new arrays."""
    next_pts = np.array(next_pts, dtype=F, copy=True)
    status = None if status is None else np.array(status, dtype=np.uint8, copy=True)
    err = None if err is None else np.array(err, dtype=F, copy=True)
    n, cap = prev_pts.shape[0], prev_pts.shape[1]
    for f in range(n):
        for i in range(min(int(counts[f]), cap)):
            out, st, e, _ = lk_point(prev[f], nxt[f], level, prev_pts[f, i], next_pts[f, i], win, max_iterations, epsilon, min_eig_threshold, use_initial)
            next_pts[f, i] = out
            if level == 0:
                if status is not None:
                    status[f, i] = st
                if err is not None:
                    err[f, i] = e
    return next_pts, status, err


def optical_flow(prev, nxt, points, counts, win=21, levels=3, max_iterations=30, epsilon=0.01, min_eig_threshold=1e-4, initial=None):
    """The whole chain of Context.optical_flow on host arrays (n, h, w): (next_pts, status, err)"""
    n = prev.shape[0]
    pp = [pyramid(prev[f], levels) for f in range(n)]
    pn = [pyramid(nxt[f], levels) for f in range(n)]
    top = len(pp[0]) - 1
    points = np.asarray(points, dtype=F)
    next_pts = np.array(points if initial is None else initial, dtype=F, copy=True)
    status = np.zeros(points.shape[:2], dtype=np.uint8)
    err = np.zeros(points.shape[:2], dtype=F)
    for lv in range(top, -1, -1):
        a = np.stack([pp[f][lv] for f in range(n)])
        b = np.stack([pn[f][lv] for f in range(n)])
        use_initial = 1 if (lv < top or initial is not None) else 0
        next_pts, status, err = lk_level(a, b, lv, counts, points, next_pts, win, max_iterations, epsilon, min_eig_threshold, use_initial, status, err)
    return next_pts, status, err
