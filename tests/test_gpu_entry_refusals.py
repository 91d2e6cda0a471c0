"""The view refusals of the four entry points that have no table of their own elsewhere: hc_run_device,
hc_run_gradients_device, hc_canny_device (a Mode O context) and hc_hysteresis_device (a Mode R one), 64 x 16, max_batch 2.
Every refused call is HC_E_ARG ("error -1") with the entry's name in its text, returns before anything is queued -- the
canary in the output buffer survives sync() -- and leaves the context fit for the valid call that follows, which gives the
oracle's maps.  The rules themselves (cudacam_amd/csrc/host_plan.h: check_view) are swept on the CPU by
tests/cpp/plan_driver.cpp; this file checks that each entry asks them of each of its views."""
import numpy as np
import pytest

from cudacam_amd import api, synth
import canny_o_ext_ref as X

pytestmark = pytest.mark.gpu

W, H, NB = 64, 16, 2
FS = W * H
CANARY = 0x5A


def _refused(entry, call, cases, d_out, ctx):
    """Each case is the valid argument tuple with some arguments replaced."""
    import torch
    for what, args in cases:
        with pytest.raises(api.HipCannyError) as ei:
            call(*args)
        assert "error -1:" in str(ei.value) and entry in str(ei.value), f"{entry}, {what}: {ei.value}"
    ctx.sync()
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == CANARY).all(), f"{entry}: a refused call wrote its output"


def _u8_cases(ok):
    """ok = (d_in, in_pitch, in_fs, d_out, out_pitch, out_fs, nframes, ...)"""
    def w(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return tuple(a)
    return [("in pitch below a row", w(_1=ok[1] - 1)), ("out pitch below a row", w(_4=W - 1)),
            ("in frame stride below a frame", w(_2=ok[1] * H - 1)), ("out frame stride below a frame", w(_5=FS - 1)),
            ("nframes 0", w(_6=0)), ("nframes -1", w(_6=-1)), ("nframes 3", w(_6=NB + 1))]


def test_mode_o_entries(oracle):
    import torch
    frames = np.stack([synth.natural(W, H, 31), synth.noise(W, H, 32)])
    grads = [X.sobel_o(f, 3) for f in frames]
    dx, dy = (np.stack([g[k] for g in grads]).astype(np.int16) for k in (0, 1))
    d_in = torch.from_numpy(frames).cuda()
    # int16 planes with two spare bytes behind, so that an odd base address stays inside the allocation
    t_dx, t_dy = (torch.from_numpy(np.concatenate([v.reshape(-1), np.zeros(1, np.int16)])).cuda() for v in (dx, dy))
    d_out = torch.full((NB, H, W), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pi, px, py, po = d_in.data_ptr(), t_dx.data_ptr(), t_dy.data_ptr(), d_out.data_ptr()
    row16 = 2 * W

    def maps():
        ctx.sync()
        got = d_out.cpu().numpy()
        d_out.fill_(CANARY)
        torch.cuda.synchronize()
        return got

    with api.Context(W, H, 1, NB, api.MODE_O) as ctx:
        ok = (pi, W, FS, po, W, FS, NB)
        _refused("hc_run_device", ctx.run_device, _u8_cases(ok), d_out, ctx)
        ok_c = ok + (60.0, 140.0)
        _refused("hc_canny_device", ctx.canny_device, _u8_cases(ok_c), d_out, ctx)
        ok_g = (px, py, row16, row16 * H, po, W, FS, NB)

        def g(**kw):
            a = list(ok_g)
            for k, v in kw.items():
                a[int(k[1:])] = v
            return tuple(a)
        cases = [("gradient pitch below a row", g(_2=row16 - 2)), ("out pitch below a row", g(_5=W - 1)),
                 ("gradient frame stride below a frame", g(_3=row16 * H - 2)), ("out frame stride below a frame", g(_6=FS - 1)),
                 ("odd dx address", g(_0=px + 1)), ("odd gradient pitch", g(_2=row16 + 1, _3=(row16 + 1) * H)),
                 ("nframes 0", g(_7=0)), ("nframes -1", g(_7=-1)), ("nframes 3", g(_7=NB + 1))]
        _refused("hc_run_gradients_device", ctx.run_gradients_device, cases, d_out, ctx)
        assert ctx.hysteresis_schedule() == dict.fromkeys(api.SCHEDULE_FIELDS, 0)   # nothing has run so far
        # one valid call per entry
        ctx.run_device(*ok)
        assert np.array_equal(maps(), np.stack([oracle.canny_o(f, 50, 150) for f in frames])), "hc_run_device"
        ctx.canny_device(*ok_c)
        assert np.array_equal(maps(), np.stack([oracle.canny_o(f, 60, 140) for f in frames])), "hc_canny_device"
        ctx.run_gradients_device(*ok_g)
        assert np.array_equal(maps(), np.stack([X.canny_o_from_gradients(a, b, 50, 150) for a, b in zip(dx, dy)])), "hc_run_gradients_device"


def test_hysteresis_entry(oracle):
    import torch
    thr = np.stack([synth.thresh_map_random(W, H, 41), synth.thresh_map_random(W, H, 42, p_cand=0.5)])
    d_thr = torch.from_numpy(thr).cuda()
    d_out = torch.full((NB, H, W), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ok = (d_thr.data_ptr(), W, FS, d_out.data_ptr(), W, FS, NB)
    with api.Context(W, H, 1, NB) as ctx:
        _refused("hc_hysteresis_device", ctx.hysteresis_device, _u8_cases(ok), d_out, ctx)
        assert ctx.hysteresis_schedule() == dict.fromkeys(api.SCHEDULE_FIELDS, 0)
        ctx.hysteresis_device(*ok)
        ctx.sync()
        assert np.array_equal(d_out.cpu().numpy(), np.stack([oracle.hysteresis(m) for m in thr]))
