"""The 8-px front kernels at every run length, remainder and height: k_front8 (form 2; mono, mono with the dense path
forced, BGR -> grey, per-channel), its half-strip form (form 4, the same four), k_front8o (form 3; L1 and L2) and the
opt-in k_front_mx (form 5).  All of them cut a frame into runs of rows and every run restarts from nothing -- warm-up
rows, a prefetch that reaches past the run, windows of six rows (blocks of 16 for k_front_mx) whose first and last rows
belong to the neighbouring runs or lie below the frame.  The automatic split gives small batches runs of 8 or 14 rows, so
this file sets the length itself (hc_set_tuning); what plan_front makes of each length is pinned in
tests/cpp/plan_driver.cpp, since the GPU cannot report it.

* leg A: every height 1 .. 22 at the form's provisional-map width (two strips), a fresh context per height, set lengths
  2, 8, 14 and 0: every last-run length 1 .. the run length, one to eleven runs per strip, frames inside one warm-up or
  one window; k_front_mx: heights and lengths from front_mx_run_rows instead (front8_runs_inputs.MX_LEG_A: last runs of
  1 .. 16 rows, runs of 12 | 13 and 28 | 29 rows); then 5 columns at heights 1, 2, 3, 7 and 8;
* leg B: 41 rows at the strip width, the provisional-map width and a second strip of one column, every distinct run length;
* pipelined: 41 rows at the provisional-map width, three device runs into two stale-filled outputs used in turn -- a row
  that no run writes into the provisional map shows.

Bit for bit against the oracle: the fast path's own blur (Mode R) and bit planes (hc_debug_tap) and the final maps.
Batches of three different frames (natural, noise, diagonal stripes; three different planes per 3-channel frame), so a
wrong frame index shows.  Before its first GPU call every case asserts, on the reference alone, that every row of every
map of every batch holds a candidate and an empty pixel -- every seam has something to get wrong.  At 5 columns that
holds for heights 1 and 2 only (Mode O: 1 and 3); at heights 3, 7, 8 (Mode O: 2, 7, 8) every map holds both somewhere
(front8_runs_inputs.PER_FRAME_RULE; tests/test_front8_runs_inputs_cpu.py asserts the same without a GPU)."""
import pytest

from cudacam_amd import api
import front8_runs_inputs as I
from test_gpu_parity import _diff

pytestmark = pytest.mark.gpu

NB = 3   # frames per batch


def _ctx(form, w, h, taps):
    ctx = api.Context(w, h, form.ch, NB, api.MODE_O if form.mode == "O" else api.MODE_R)
    try:
        if form.mode == "O":
            ctx.set_option(api.OPT_L2_GRADIENT, int(form.l2))
        else:
            if form.per_channel:
                ctx.set_option(api.OPT_PER_CHANNEL, 1)
            ctx.set_option(api.OPT_FRONT_HALF, 1 if form.kernel == "half" else 0)
            if form.dense:
                ctx.set_option(api.OPT_FRONT_DENSE, 1)
            if form.kernel == "mx":
                ctx.set_option(api.OPT_FRONT_MX, 1)
        ctx.set_thresholds(*I.THRESHOLDS[form.mode])
        if taps:
            ctx.set_option(api.OPT_DEBUG_TAPS, 1)
    except Exception:
        ctx.close()
        raise
    return ctx


def _plain(oracle, form, w, h, lengths):
    """One context; every set length in turn, both batches: blur, bit planes, edges."""
    refs = I.references(oracle, form, w, h)
    with _ctx(form, w, h, taps=True) as ctx:
        for c in lengths:
            ctx.set_tuning(c, 0)
            for k, r in enumerate(refs):
                what = f"{form.name} {w}x{h}, set length {c}, batch {k}"
                got = ctx.process(r.frames)
                assert ctx.last_run_info()[2] == form.front_form, what
                n = len(r.pre)
                if r.blur is not None:
                    _diff(ctx.debug_tap(api.TAP_BLUR, n), r.blur, what + ": blur")
                _diff(ctx.debug_tap(api.TAP_THRESH, n), r.pre, what + ": bit planes")
                _diff(got, r.edges, what + ": edges")


def _pipelined(oracle, form, w, h, lengths):
    """Per set length three runs (batches 0, 1, 1) into two outputs used in turn; the last two maps are checked, then both
    outputs get stale bytes again.  Run 1 writes over stale bytes and run 2 over the map of another batch, so a row that
    either leaves out shows."""
    import torch
    refs = I.references(oracle, form, w, h)
    n_out = len(refs[0].pre)
    d_in = [torch.from_numpy(r.frames).cuda() for r in refs]
    d_out = [torch.full((n_out, h, w), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(2)]
    seq = (0, 1, 1)
    with _ctx(form, w, h, taps=False) as ctx:
        ctx.set_option(api.OPT_PIPELINE, 1)
        for c in lengths:
            ctx.set_tuning(c, 0)
            torch.cuda.synchronize()   # the context's stream does not wait for the fills
            for r, k in enumerate(seq):
                ctx.run_device(d_in[k].data_ptr(), w * form.ch, w * form.ch * h, d_out[r % 2].data_ptr(), w, w * h, NB)
            ctx.sync()
            assert ctx.last_run_info() == (False, False, form.front_form)
            for r in (1, 2):
                _diff(d_out[r % 2].cpu().numpy(), refs[seq[r]].edges, f"{form.name} {w}x{h}, set length {c}, pipelined run {r}")
                d_out[r % 2].fill_(0x5A + r)


@pytest.mark.parametrize("form", I.FORMS, ids=[f.name for f in I.FORMS])
def test_every_run_length_remainder_and_height(oracle, form):
    for w, h in I.shapes(form):
        I.assert_not_vacuous(oracle, form, w, h)
    for w, h, lengths in I.leg_a(form) + I.leg_b(form):
        _plain(oracle, form, w, h, lengths)
    w, h, lengths = I.leg_b(form)[1]
    assert w % 8 == 0   # the front kernel writes the provisional map
    _pipelined(oracle, form, w, h, lengths)
