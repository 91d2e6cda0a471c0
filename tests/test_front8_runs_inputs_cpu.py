"""The inputs of tests/test_gpu_front8_runs.py (tests/front8_runs_inputs.py) against the oracle, without a GPU: for every
(form, shape, batch) the reference's tri-state map holds a candidate and an empty pixel in every row of every map -- at 5
columns, where listed, in every map -- so a seed that stops working fails here; and the set lengths really give the runs
the GPU file is about (the cut functions restate plan_front; tests/cpp/plan_driver.cpp pins plan_front itself)."""
import os
import re

import numpy as np
import pytest

import front8_runs_inputs as I


@pytest.mark.parametrize("form", I.FORMS, ids=[f.name for f in I.FORMS])
def test_every_seam_has_something_to_get_wrong(oracle, form):
    for w, h in I.shapes(form):
        I.assert_not_vacuous(oracle, form, w, h)
        for r in I.references(oracle, form, w, h):
            n_out = 3 * len(r.frames) if form.per_channel else len(r.frames)
            assert r.pre.shape == r.edges.shape == (n_out, h, w) and (r.blur is None) == (form.mode == "O")
            assert len({f.tobytes() for f in r.frames}) == len(r.frames) == 3, "three different frames"
            if form.ch == 3 and h > 1:
                assert all(len({np.ascontiguousarray(f[:, :, c]).tobytes() for c in range(3)}) == 3 for f in r.frames), "three different planes"


def test_the_rule_can_fail():
    assert I.vacuous(np.zeros((1, 2, 5), np.uint8)) and I.vacuous(np.full((1, 2, 5), 128, np.uint8), per_frame=True)
    mixed = np.array([[[0, 128, 0], [0, 0, 0]]], np.uint8)
    assert I.vacuous(mixed) and not I.vacuous(mixed, per_frame=True) and not I.vacuous(mixed[:, :1])
    assert all(w == I.TINY_W for _, w, _ in I.PER_FRAME_RULE)


def test_set_lengths_reach_every_run_and_remainder():
    # k_front8 / k_front8o, leg A: run lengths 2, 8 and 14 with every last-run length 1 .. the run length, one to eleven runs
    seen = {}
    for h in I.LEG_A_HEIGHTS:
        for c in I.LEG_A_LENGTHS[:3]:
            run, runs, last = I.front8_cut(h, c)
            seen.setdefault(run, set()).add((runs, last))
    assert sorted(seen) == [2, 8, 14]
    for run, v in seen.items():
        assert {last for _, last in v} == set(range(1, run + 1)), run
    assert {runs for runs, _ in seen[2]} == set(range(1, 12))
    # leg B: every distinct run length of 41 rows, then one run
    assert [I.front8_cut(I.H_B, c)[:2] for c in I.LEG_B_LENGTHS] == [(2, 21), (8, 6), (14, 3), (20, 3), (26, 2), (32, 2), (38, 2), (44, 1), (44, 1)]
    assert {6 * k - 4 for k in range(1, 8)} == {I.front8_cut(I.H_B, c)[0] for c in I.LEG_B_LENGTHS[:7]}
    # k_front_mx, leg A: a last run of every length 1 .. 16 behind another run; both sides of the block borders
    cuts = [I.mx_cut(h, c) for h, cs in I.MX_LEG_A.items() for c in cs if c]
    assert {last for _, runs, last in cuts if runs > 1} >= set(range(1, 17))
    borders = [I.front_mx_run_rows(b) for b in (1, 2)]
    assert borders == [12, 28]
    for r in borders:
        assert {(r, 2, r), (r + 1, 2, r), (r + 1, 2, r + 1), (r, 3, r), (r + 1, 3, r + 1)} <= set(cuts), r
    # leg B: every run length that 41 rows can be cut into
    assert {I.mx_cut(I.H_B, c)[0] for c in I.MX_LEG_B_LENGTHS} == {(I.H_B + k - 1) // k for k in range(1, I.H_B + 1)}
    assert [I.mx_cut(I.H_B, c)[0] for c in I.MX_LEG_B_LENGTHS[:-1]] == list(I.MX_LEG_B_LENGTHS[:-1])


def test_geometry_restated_here_is_the_kernels():
    """The constants the helper restates are those of cudacam_amd/csrc/canny_params.h."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cudacam_amd", "csrc", "canny_params.h")
    with open(path) as f:
        src = f.read()

    def const(name):
        return re.search(r"constexpr int %s = ([^;]+);" % name, src).group(1).strip()
    assert (const("MX_ROWS"), const("MX_LAG"), const("MX_STRIP_W"), const("F8_SUB")) == (str(I.MX_ROWS), str(I.MX_LAG), str(I.WIDTHS["mx"][0]), "6")
    assert const("F8_STRIP_W") == "62 * 8" and const("F8_HSTRIP_W") == "30 * 8" and (I.WIDTHS["f8"][0], I.WIDTHS["half"][0]) == (496, 240)
    assert "inline int front_mx_run_rows(int blocks) { return MX_ROWS * blocks - MX_LAG; }" in src
    assert "inline int front8_run_rows(int windows) { return F8_SUB * windows - 4; }" in src
