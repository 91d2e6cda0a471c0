"""Caller views on every entry point: pitched rows, offset bases, frame gaps and ROIs of a larger parent, on the input and
on the output side, for every front form, plain and pipelined -- against the oracle, bit for bit, with every byte outside
the output view checked for survival (tests/view_arena.py).  Everything here is integer and exact: no tolerances.

Geometry families (pitches in bytes, rb = row bytes of the input, w8 = round_up(W, 8)):
  T      tight rows, allocator-aligned base (the control; tight rows of a width that is not a multiple of 8 are staged)
  P4     in_pitch = w8 * C + 4, out_pitch = w8 + 4 (both = 4 mod 8), bases +4 / +12, frame strides pitch * H + 20:
         everything a multiple of 4, nothing of 8 or 16 -- in place, no staging
  GM     GpuMat-like: out_pitch = round_up(W, 512), in_pitch = round_up(rb, 512) + 512
  ROI    a rectangle at (y0, x0) of a parent image, x0 * C = 4 mod 16, neighbours = the parent's pixels; the output is an
         ROI of another parent with another pitch and offset
  MIXI / MIXO   input padded (P4) and output tight, and the reverse
  ODDI / ODDO / ODDB   an odd base and pitch on the input, the output, both: staged exactly as hipcanny.h promises
  G2     (gradient entry only) int16 planes at a pitch = 2 mod 4 and a base = 2 mod 4, output padded as P4
The 8-px kernels load the columns W .. w8 - 1 of padded rows: with fill "random" / "ff" / "parent" those bytes are
garbage, all-255 or a neighbour's pixels, and must not change a result (Mode R substitutes zeros, Mode O the border).
"""
import ctypes as C

import numpy as np
import pytest

from cudacam_amd import api, synth
import canny_o_ext_ref as X
import view_arena as VA

pytestmark = pytest.mark.gpu

HEIGHTS = (1, 2, 5, 37, 83)
GIB4 = 1 << 32


# ---------------------------------------------------------------------------------------------------------------------
# geometry families
# ---------------------------------------------------------------------------------------------------------------------
def _roi_x0(bpp):
    """Smallest column >= 2 whose byte offset is 4 mod 16."""
    return next(x for x in range(2, 64) if (x * bpp) % 16 == 4)


def _in_family(fam, w, h, bpp):
    """(pitch, frame_stride, base_off, fill or None) of the input view; bpp = bytes per pixel (C, or 2 C for int16)."""
    rb, w8 = w * bpp, VA.round_up(w, 8)
    if fam in ("T", "MIXO", "ODDO"):
        if fam == "ODDO" and w % 8:   # (tight ragged rows would be staged: keep the input in place, the case is the output)
            return w8 * bpp + 4, (w8 * bpp + 4) * h + 20, 4, None
        return rb, rb * h, 0, None
    if fam in ("P4", "MIXI"):
        p = w8 * bpp + 4
        return p, p * h + 20, 4, None
    if fam == "GM":
        p = VA.round_up(rb, 512) + 512
        return p, p * h, 0, None
    if fam == "ROI":
        x0, y0 = _roi_x0(bpp), 3
        p = VA.round_up((w + x0 + 23) * bpp, 4)
        return p, p * (h + y0 + 4), y0 * p + x0 * bpp, "parent"
    if fam in ("ODDI", "ODDB"):
        p = w8 * bpp + 1
        return p, p * h + 3, 1, None
    if fam == "G2":
        p = rb + 2 if rb % 4 == 0 else rb + 4
        return p, p * h + 2, 2, None
    raise ValueError(fam)


def _out_family(fam, w, h):
    """(pitch, frame_stride, base_off) of the output view."""
    w8 = VA.round_up(w, 8)
    if fam in ("T", "MIXI", "ODDI"):
        return w, w * h, 0
    if fam in ("P4", "MIXO", "G2"):
        p = w8 + 4
        return p, p * h + 20, 12
    if fam == "GM":
        p = VA.round_up(w, 512)
        return p, p * h, 0
    if fam == "ROI":
        x0, y0 = 36, 2
        p = VA.round_up(w + x0 + 17, 4)
        return p, p * (h + y0 + 3), y0 * p + x0
    if fam in ("ODDO", "ODDB"):
        p = VA.round_up(w, 4) + 1
        return p, p * h + 1, 3
    raise ValueError(fam)


def _lead(pitch):
    """A lead of whole 512-byte blocks: the view's alignment is then that of its base offset (torch allocates at 512)."""
    return VA.round_up(pitch + 64, 512)


FAMILIES = ("T", "P4", "GM", "ROI", "MIXI", "MIXO", "ODDI", "ODDO", "ODDB")
# hc_run_gradients_device takes even addresses and pitches only (odd ones are HC_E_ARG, nothing is staged on its input side)
GRAD_FAMILIES = ("T", "P4", "GM", "ROI", "MIXI", "MIXO", "ODDO", "G2")


# ---------------------------------------------------------------------------------------------------------------------
# forms
# ---------------------------------------------------------------------------------------------------------------------
class Form:
    def __init__(self, name, mode, ch, widths, form, opts=(), front_split=None, low=None, high=None, kind="u8", aperture=3, l2=False,
                 per_channel=False, families=FAMILIES):
        self.name, self.mode, self.ch, self.widths, self.form, self.opts, self.front_split = name, mode, ch, widths, form, opts, front_split
        self.low = low if low is not None else (10 if mode == api.MODE_R else 50)
        self.high = high if high is not None else (40 if mode == api.MODE_R else 150)
        self.kind, self.aperture, self.l2, self.per_channel, self.families = kind, aperture, l2, per_channel, families

    @property
    def wants8(self):   # hipcanny.h: rows without whole 8-pixel groups are staged so that the 8-px kernels can run
        split2 = self.front_split in (None, 2)
        return split2 and (self.mode == api.MODE_R or self.ch == 1) and self.aperture == 3 and self.kind == "u8"


R, O = api.MODE_R, api.MODE_O
FORMS = [
    # Mode R
    Form("front8", R, 1, (1, 5, 29, 495, 496, 497, 504, 641, 1000, 2049), 2, opts=((api.OPT_FRONT_HALF, 0),)),
    Form("half", R, 1, (3, 29, 239, 240, 241, 480), 4, opts=((api.OPT_FRONT_HALF, 1),)),
    Form("dense", R, 1, (29, 496, 497, 641), 2, opts=((api.OPT_FRONT_HALF, 0), (api.OPT_FRONT_DENSE, 1))),
    Form("mx", R, 1, (5, 215, 216, 217, 640, 1000, 2047), 5, opts=((api.OPT_FRONT_MX, 1),)),
    Form("bgr", R, 3, (3, 241, 497, 640), 2, opts=((api.OPT_FRONT_HALF, 0),)),
    Form("per_channel", R, 3, (5, 241, 496), 2, opts=((api.OPT_FRONT_HALF, 0), (api.OPT_PER_CHANNEL, 1)), per_channel=True),
    Form("legacy_split", R, 1, (29, 241, 640), 1, front_split=1),
    Form("legacy_fused4", R, 1, (29, 241, 640), 0, front_split=0),
    # Mode O
    Form("front8o", O, 1, (1, 29, 495, 496, 497, 1000, 2048, 4100), 3),
    Form("front_o_bgr", O, 3, (5, 241, 640), -1),
    Form("front_o_split0", O, 1, (29, 497, 640), -1, front_split=0),
    Form("front8o_l2", O, 1, (241, 640), 3, l2=True),
    Form("aperture5", O, 1, (3, 29, 241, 640), 6, aperture=5, low=300, high=900),
    Form("aperture5_bgr", O, 3, (29, 241), 6, aperture=5, low=300, high=900),
    Form("gradients", O, 1, (1, 5, 241, 640), 7, kind="grad", families=GRAD_FAMILIES),
    Form("gradients_bgr", O, 3, (29,), 7, kind="grad", families=GRAD_FAMILIES),
]
FORM_BY_NAME = {f.name: f for f in FORMS}
CASES = [(f.name, w, fam) for f in FORMS for w in f.widths for fam in f.families]


def _content(w, h, ch, n, seed):
    """Natural and noise frames, plus one whose last column and last row are 255: a maximal gradient next to the padding."""
    def plane(k, s):
        if k % 3 == 0:
            return synth.natural(w, h, s)
        if k % 3 == 1:
            return synth.noise(w, h, s)
        img = synth.natural(w, h, s)
        img[:, -1] = 255
        img[-1, :] = 255
        return img
    out = []
    for f in range(n):
        k = seed + f
        out.append(plane(k, 11 * seed + f) if ch == 1 else np.stack([plane(k, 11 * seed + f), plane(k + 1, 7 * seed + f + 1), plane(k, 5 * seed + f + 2)[::-1].copy()], -1))
    return np.stack(out)


def _want(form, frames, oracle):
    if form.kind == "grad":
        dx, dy = frames
        return np.stack([X.canny_o_from_gradients(a, b, form.low, form.high, form.l2) for a, b in zip(dx, dy)])
    if form.mode == api.MODE_R:
        if form.per_channel:
            return np.stack([oracle.canny_r(np.ascontiguousarray(f[:, :, c]), form.low, form.high) for f in frames for c in range(3)])
        return np.stack([oracle.canny_r(f, form.low, form.high) for f in frames])
    if form.aperture == 5:
        return np.stack([X.canny_o(f, form.low, form.high, ksize=5, l2=form.l2) for f in frames])
    return np.stack([oracle.canny_o(f, form.low, form.high, l2gradient=form.l2) for f in frames])


def _device_ptrs(ctx):
    vp, sz = C.c_void_p, C.c_size_t
    a, b, ip, op, ifs, ofs = vp(), vp(), sz(), sz(), sz(), sz()
    api._ck(ctx.lib.hc_device_ptrs(ctx.handle, C.byref(a), C.byref(b), C.byref(ip), C.byref(op), C.byref(ifs), C.byref(ofs)))
    return a.value, b.value, ip.value, op.value, ifs.value, ofs.value


def _half_form_fits(ctx, form, w, h, in_fs, out_fs, piped):
    """HC_OPT_FRONT_HALF 1 is "whenever the buffers allow it": half-wave B reaches its frame by a 32-bit lane offset into
    areas the context sized from its own buffers -- max(internal input frame, 3 output frames, 3 bit-plane frames) + 32 KiB,
    in whole pages.  A caller frame stride beyond that keeps the plain form (2)."""
    _, _, _, _, ifs, ofs = _device_ptrs(ctx)
    region = VA.round_up(max(ifs, 3 * ofs, 3 * 4 * 64 * h) + 32768, 4096)   # (widths up to 2048: bit-plane rows of 64 dwords)
    return in_fs + 32768 <= region and (not (piped and w % 8 == 0) or out_fs + 16384 <= region)


def _make_ctx(form, w, h, n):
    ctx = api.Context(w, h, form.ch, n, form.mode, front_split=form.front_split)
    ctx.set_thresholds(form.low, form.high)
    for opt, val in form.opts:
        ctx.set_option(opt, val)
    if form.aperture != 3:
        ctx.set_option(api.OPT_APERTURE, form.aperture)
    if form.l2:
        ctx.set_option(api.OPT_L2_GRADIENT, 1)
    return ctx


@pytest.mark.parametrize("name,w,fam", CASES, ids=[f"{a}-{b}-{c}" for a, b, c in CASES])
def test_front_forms_on_views(oracle, name, w, fam):
    """One form, one width, one geometry family: input fill "random" and "ff" (ROI: the parent's pixels and "ff"), a plain
    run and three pipelined runs into two output arenas in turn; maps exact, guards intact in both arenas, form and staging
    as hc_last_run_info promises."""
    import torch
    form = FORM_BY_NAME[name]
    k = form.widths.index(w) + form.families.index(fam) + len(name)
    h, n = HEIGHTS[k % 5], (3 if k % 2 else 1)
    grad = form.kind == "grad"
    bpp = form.ch * (2 if grad else 1)
    n_out = 3 * n if form.per_channel else n
    base = _content(w, h, form.ch, n, k)
    seq, want = [], []
    for r in range(3):   # the three pipelined runs; the plain run takes the input of the last
        fr = np.stack([np.roll(f, 7 * (r + 1), axis=0) for f in base]) if h > 1 else np.stack([np.roll(f, 3 * (r + 1), axis=1) for f in base])
        if grad:
            g = [X.sobel_o(f, 3) for f in fr]
            fr = (np.stack([a for a, _ in g]).astype(np.int16), np.stack([b for _, b in g]).astype(np.int16))
        seq.append(fr)
        want.append(_want(form, fr, oracle) if r else None)   # (run 0's map is overwritten by run 2's)
    ip, ifs, ioff, ifill = _in_family(fam, w, h, bpp)
    op, ofs, ooff = _out_family(fam, w, h)
    in_aligned = (ioff | ip | ifs) % (2 if grad else 4) == 0
    exp_in = (not grad) and (not in_aligned or (form.wants8 and ip < VA.round_up(w, 8) * form.ch)
                             or (form.mode == api.MODE_O and (form.ch == 3 or form.aperture == 5) and ip < VA.round_up(w, 4) * form.ch))
    exp_out = (ooff | op | ofs) % 4 != 0
    if fam == "P4" or fam == "ROI":
        assert not exp_in and not exp_out, "these families run in place"
    if fam in ("ODDI", "ODDB"):
        assert exp_in or grad
    if fam in ("ODDO", "ODDB"):
        assert exp_out
    with _make_ctx(form, w, h, n) as ctx:
        for fill in ((ifill or "random"), "ff"):
            d_in = []
            for r in range(3):
                planes = seq[r] if grad else (seq[r],)
                d_in.append([torch.from_numpy(VA.make_input(p, ip, ifs, ioff, fill, lead=_lead(ip), seed=k + r + 10 * j)[0]).cuda() for j, p in enumerate(planes)])
            in_off = _lead(ip) + ioff
            before = [VA.make_output(n_out, h, w, op, ofs, ooff, lead=_lead(op), seed=k + j) for j in range(2)]
            go = before[0][1]

            def run(r, d_out):
                a = d_in[r]
                if grad:
                    ctx.run_gradients_device(a[0].data_ptr() + in_off, a[1].data_ptr() + in_off, ip, ifs, d_out.data_ptr() + go.offset, op, ofs, n)
                else:
                    ctx.run_device(a[0].data_ptr() + in_off, ip, ifs, d_out.data_ptr() + go.offset, op, ofs, n)

            for piped in (0, 1):
                ctx.set_option(api.OPT_PIPELINE, piped)
                d_out = [torch.from_numpy(b[0]).cuda() for b in before]
                torch.cuda.synchronize()
                if piped:
                    for r in range(3):
                        run(r, d_out[r % 2])
                else:
                    run(2, d_out[0])
                ctx.sync()
                exp_form = form.form
                if name == "half" and not _half_form_fits(ctx, form, w, h, ifs if not exp_in else 0, ofs if not exp_out else 0, piped):
                    exp_form = 2
                what = f"{name} {w}x{h}x{form.ch} n {n} {fam} fill {fill} {'pipelined' if piped else 'plain'}"
                assert ctx.last_run_info() == (exp_in, exp_out, exp_form), f"{what}: (input staged, output staged, form) = {ctx.last_run_info()}"
                VA.check_output(d_out[0].cpu().numpy(), before[0][0], go, want[2], what + ", arena 0")
                if piped:
                    VA.check_output(d_out[1].cpu().numpy(), before[1][0], go, want[1], what + ", arena 1")
                else:
                    assert np.array_equal(d_out[1].cpu().numpy(), before[1][0])


# ---------------------------------------------------------------------------------------------------------------------
# hc_hysteresis_device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["P4", "GM", "ROI"])
@pytest.mark.parametrize("w,h,n", [(29, 5, 3), (241, 37, 1), (640, 83, 3), (2049, 37, 1), (5, 1, 1)])
def test_hysteresis_device_on_views(oracle, w, h, n, fam):
    """Tri-state maps whose padding holds 255 and 128: strong and candidate bytes one past the last column, before the
    first, and in the rows around the view must not seed or carry an edge."""
    import torch
    maps = np.stack([synth.thresh_map_random(w, h, 5 + f + w) if f % 2 == 0 or w < 40 or h < 20 else synth.thresh_map_serpentine(w, h) for f in range(n)])
    maps[:, :, -1] = np.where(maps[:, :, -1] == 0, 128, maps[:, :, -1])   # candidates in the last column, next to the strong padding
    maps[:, -1, :] = np.where(maps[:, -1, :] == 0, 128, maps[:, -1, :])
    want = np.stack([oracle.hysteresis(m) for m in maps])
    ip, ifs, ioff, _ = _in_family(fam, w, h, 1)
    op, ofs, ooff = _out_family(fam, w, h)
    arena, off = VA.make_input(maps, ip, ifs, ioff, "random", lead=_lead(ip), seed=w)
    gi = VA.input_geometry(maps, ip, ifs, ioff, lead=_lead(ip))
    outside = ~gi.inside()
    arena[outside] = np.where(arena[outside] & 1, 255, 128).astype(np.uint8)
    st = gi.row_starts()
    assert arena[st[0, 0] + w] in (128, 255) and arena[st[-1, -1] + ip] in (128, 255) and (arena == 255).any() and (arena == 128).any()
    before, go = VA.make_output(n, h, w, op, ofs, ooff, lead=_lead(op), seed=w + 1)
    d_in, d_out = torch.from_numpy(arena).cuda(), torch.from_numpy(before).cuda()
    torch.cuda.synchronize()
    with api.Context(w, h, 1, n) as ctx:
        ctx.hysteresis_device(d_in.data_ptr() + off, ip, ifs, d_out.data_ptr() + go.offset, op, ofs, n)
        ctx.sync()
        VA.check_output(d_out.cpu().numpy(), before, go, want, f"hysteresis_device {w}x{h} n {n} {fam}")
        assert np.array_equal(d_in.cpu().numpy(), arena), "the input arena was written"


# ---------------------------------------------------------------------------------------------------------------------
# stage outputs below HYSTER
# ---------------------------------------------------------------------------------------------------------------------
STAGE_KEYS = {api.CannyStage.MONO: "mono", api.CannyStage.GAUSSIAN: "blur", api.CannyStage.GRADIENT: "grad_disp", api.CannyStage.NMS: "nms",
              api.CannyStage.THRESH: "thresh"}


@pytest.mark.parametrize("fam", ["P4", "ROI"])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h,n", [(29, 5, 3), (241, 37, 1), (497, 83, 1), (640, 37, 3)])
def test_stage_outputs_on_views(oracle, w, h, n, ch, fam):
    import torch
    frames = _content(w, h, ch, n, w + ch)
    stages = [oracle.canny_r(f, 10, 40, stages=True) for f in frames]
    ip, ifs, ioff, ifill = _in_family(fam, w, h, ch)
    op, ofs, ooff = _out_family(fam, w, h)
    arena, off = VA.make_input(frames, ip, ifs, ioff, ifill or "random", lead=_lead(ip), seed=3)
    d_in = torch.from_numpy(arena).cuda()
    with api.Context(w, h, ch, n) as ctx:
        for stage, key in STAGE_KEYS.items():
            before, go = VA.make_output(n, h, w, op, ofs, ooff, lead=_lead(op), seed=int(stage))
            d_out = torch.from_numpy(before).cuda()
            torch.cuda.synchronize()
            ctx.run_device(d_in.data_ptr() + off, ip, ifs, d_out.data_ptr() + go.offset, op, ofs, n, stage)
            ctx.sync()
            assert ctx.last_run_info() == (False, False, -1)
            want = np.stack([frames[f] if (ch == 1 and key == "mono") else stages[f][key] for f in range(n)])
            VA.check_output(d_out.cpu().numpy(), before, go, want, f"stage {key} {w}x{h}x{ch} n {n} {fam}")


# ---------------------------------------------------------------------------------------------------------------------
# host-side strides: hc_upload, hc_download, hc_download_begin / _end, hc_debug_tap
# ---------------------------------------------------------------------------------------------------------------------
def _ptr(a, off=0):
    return C.c_void_p(a.ctypes.data + off)


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h,n", [(640, 37, 3), (641, 37, 3), (29, 5, 1), (496, 83, 2)])
def test_host_strides(oracle, w, h, n, ch):
    """Strided and tight host views through the C ABI.  Widths of whole 16-byte rows are kept tight inside the context: a
    tight host view then takes the one-block copies, every other combination the row-by-row ones (640 / 496 against 641 / 29,
    each with a tight and a padded host view)."""
    frames = _content(w, h, ch, n, 2 * w + ch)
    stages = [oracle.canny_r(f, 10, 40, stages=True) for f in frames]
    want = np.stack([s["edges"] for s in stages])
    rb = w * ch
    with api.Context(w, h, ch, n) as ctx:
        L, hd = ctx.lib, ctx.handle
        ctx.set_option(api.OPT_DEBUG_TAPS, 1)
        for host_tight in (True, False):
            irow, ifs, ioff = (rb, rb * h, 0) if host_tight else (rb + 13, (rb + 13) * h + 77, 5)
            orow, ofs, ooff = (w, w * h, 0) if host_tight else (w + 11, (w + 11) * h + 50, 7)
            arena, off = VA.make_input(frames, irow, ifs, ioff, "random", seed=w)
            api._ck(L.hc_upload(hd, _ptr(arena, off), irow, ifs, n))
            ctx.run(api.CannyStage.HYSTER, n)
            what = f"{w}x{h}x{ch} n {n} host {'tight' if host_tight else 'strided'}"
            # hc_download
            before, go = VA.make_output(n, h, w, orow, ofs, ooff, seed=1)
            after = before.copy()
            api._ck(L.hc_download(hd, _ptr(after, go.offset), orow, ofs, n))
            VA.check_output(after, before, go, want, "hc_download " + what)
            # hc_download_begin / _end into page-locked memory
            pinned = L.hc_host_alloc(go.size)
            assert pinned
            try:
                pin = np.frombuffer((C.c_uint8 * go.size).from_address(pinned), np.uint8)
                pin[:] = before
                api._ck(L.hc_download_begin(hd, C.c_void_p(pinned + go.offset), orow, ofs, n))
                api._ck(L.hc_download_end(hd))
                VA.check_output(pin.copy(), before, go, want, "hc_download_begin/_end " + what)
                del pin
            finally:
                L.hc_host_free(pinned)
            # hc_debug_tap, both taps
            for tap, key in ((api.TAP_BLUR, "blur"), (api.TAP_THRESH, "thresh")):
                after = before.copy()
                api._ck(L.hc_debug_tap(hd, tap, _ptr(after, go.offset), orow, ofs, n))
                VA.check_output(after, before, go, np.stack([s[key] for s in stages]), f"hc_debug_tap {key} " + what)
        with pytest.raises(api.HipCannyError):
            api._ck(L.hc_upload(hd, _ptr(arena, off), rb - 1, ifs, n))
        with pytest.raises(api.HipCannyError):
            api._ck(L.hc_download(hd, _ptr(after, go.offset), w - 1, ofs, n))


# ---------------------------------------------------------------------------------------------------------------------
# views of 4 GiB and more
# ---------------------------------------------------------------------------------------------------------------------
def _free_gib():
    import torch
    return torch.cuda.mem_get_info()[0] / (1 << 30) if torch.cuda.is_available() else 0


@pytest.mark.parametrize("side", ["out_front8", "out_mx", "in_front8", "in_mx"])
def test_views_of_4gib(oracle, side):
    """W = 640, H = 1100, one frame, pipelined, one side at a pitch of 4 MiB: H * pitch > 2^32.

    Output side: the front kernels place the rows of the provisional map with 32-bit offsets; before the fix row 1024 of
    the map landed on row 0 (1024 * 4 MiB = 2^32) and rows 1025.. on the rows after it, so rows 0..75 showed the strong
    pixels of rows 1024..1099 and rows 1024.. kept whatever the buffer held.  Such a view now gets no provisional map
    (the hysteresis, with 64-bit offsets, writes the whole map).  Input side: the launchers refused the view
    (hipErrorInvalidValue, a hard failure of the run); it is now staged through the internal buffer and reported."""
    import torch
    if _free_gib() < 12:
        pytest.skip("needs 12 GiB of free device memory")
    w, h, pitch = 640, 1100, 4 << 20
    assert h * pitch > GIB4
    img = synth.natural(w, h, 77)
    img[1024:1030, 100:300] = 255   # strong edges in the rows that used to wrap onto rows 0..5
    want = oracle.canny_r(img, 10, 40)
    assert want[1023:1031].any() and not np.array_equal(want[0:8], want[1024:1032])
    big = torch.empty(h * pitch + 4096, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(big, (h, pitch), (pitch, 1))
    mx = side.endswith("mx")
    with api.Context(w, h, 1, 1) as ctx:
        ctx.set_option(api.OPT_FRONT_HALF, 0)
        ctx.set_option(api.OPT_FRONT_MX, 1 if mx else 0)
        ctx.set_option(api.OPT_PIPELINE, 1)
        if side.startswith("out"):
            d_in = torch.from_numpy(img).cuda()
            view[:, :w + 64] = 7   # the view and a guard band of 64 columns beside it
            torch.cuda.synchronize()
            ctx.run_device(d_in.data_ptr(), w, w * h, big.data_ptr(), pitch, pitch * h, 1)
            ctx.sync()
            assert ctx.last_run_info() == (False, False, 5 if mx else 2)
            got = view[:, :w + 64].cpu().numpy()
            bad = np.flatnonzero((got[:, :w] != want).any(axis=1))
            assert bad.size == 0, f"{side}: {bad.size} rows differ, first row {int(bad[0])}"
            assert (got[:, w:] == 7).all(), "bytes beside the view were written"
        else:
            view[:, :w] = torch.from_numpy(img).cuda()
            d_out = [torch.full((h, w), 7, dtype=torch.uint8, device="cuda") for _ in range(2)]
            torch.cuda.synchronize()
            for r in range(2):
                ctx.run_device(big.data_ptr(), pitch, pitch * h, d_out[r].data_ptr(), w, w * h, 1)
            ctx.sync()
            assert ctx.last_run_info() == (True, False, 5 if mx else 2)
            for r in range(2):
                bad = np.flatnonzero((d_out[r].cpu().numpy() != want).any(axis=1))
                assert bad.size == 0, f"{side}: run {r}: {bad.size} rows differ, first row {int(bad[0])}"
    del view, big
    torch.cuda.empty_cache()
