"""The C++ drop-in surface (include/cvp/*.hpp over the C ABI)."""
import os
import subprocess

import numpy as np
import pytest

from cudacam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cudacam_amd", "libcvProcessing_hip.so")
BIN = os.path.join(ROOT, "tests", "cpp", "test_cvpipeline")


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cudacam_amd", "csrc")])


def test_cpp_surface_builds_and_exports():
    """CPU: the header-compatible classes compile against include/cvp and export the reference's members."""
    from cudacam_amd import build
    build.build()
    _build()
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", LIB], text=True)
    # cv::Mat never crosses the boundary (include/cvp/frameView.hpp): the Mat-taking members are inline
    # wrappers in the headers, the library exports the view forms and no symbol that mentions cv::Mat
    assert "cv::Mat" not in syms, [l for l in syms.splitlines() if "cv::Mat" in l]
    for want in ("cvp::cvPipeline::processView(cvp::FrameView const&, cvp::CannyStage)", "cvp::cvPipeline::setLowThreshold(unsigned char)",
                 "cvp::cvPipeline::getHighThreshold() const", "cvp::cvPipeline::enableCudaProfiling(bool)",
                 "cvp::cvPipeline::isCudaProfilingEnabled() const", "cvp::cuda::CannyEdge::runView(cvp::FrameView const&, cvp::CannyStage)",
                 "cvp::cuda::CannyEdge::CannyEdge(unsigned int, unsigned int, unsigned int, int)"):
        assert want in syms, want


@pytest.mark.gpu
@pytest.mark.parametrize("binary", ["test_cvpipeline", "test_cvpipeline_othermat"])
@pytest.mark.parametrize("channels,stage", [(1, 5), (3, 5), (1, 3), (3, 2), (3, 0), (1, 0), (3, 4)])
def test_cpp_pipeline_matches_oracle(oracle, tmp_path, channels, stage, binary):
    """`test_cvpipeline_othermat` is the same driver built against a cv::Mat with OpenCV's member order
    (tests/cpp/other_mat_layout): the host's Mat layout must not matter to the prebuilt library."""
    BIN = os.path.join(ROOT, "tests", "cpp", binary)
    if not os.path.exists(BIN):
        _build()
    w, h = 321, 200
    img = synth.natural(w, h, 77) if channels == 1 else np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
    fin, fout = tmp_path / "in.raw", tmp_path / "out.raw"
    img.tofile(fin)
    r = subprocess.run([BIN, str(w), str(h), str(channels), str(fin), str(stage), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    got = np.fromfile(fout, np.uint8).reshape(h, w)
    key = {5: "edges", 4: "thresh", 3: "nms", 2: "grad_disp", 0: "mono"}[stage]
    if stage == 5 and channels == 3:  # all six timers hold a sample
        assert r.stdout.count("samples 2") == 6, r.stdout
    assert np.array_equal(got, oracle.canny_r(img, 10, 40, stages=True)[key])


@pytest.mark.gpu
@pytest.mark.parametrize("binary", ["test_cvpipeline", "test_cvpipeline_othermat"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("w,h,x0,y0,pad", [(321, 200, 20, 3, 23), (640, 83, 4, 1, 0), (29, 5, 7, 2, 5)])
def test_cpp_pipeline_on_a_roi_of_a_parent(oracle, tmp_path, channels, binary, w, h, x0, y0, pad):
    """The driver wraps an ROI of a parent image in cv::Mat(rows, cols, type, data, step) -- a Mat that is not continuous,
    whose row padding is the parent's pixels: stage 5 of the ROI's pixels alone, against the oracle."""
    BIN = os.path.join(ROOT, "tests", "cpp", binary)
    if not os.path.exists(BIN):
        _build()
    pw, ph = x0 + w + pad, y0 + h + 4
    parent = synth.natural(pw, ph, 31) if channels == 1 else np.stack([synth.natural(pw, ph, 31 + c) for c in range(3)], -1)
    parent[y0:y0 + h, x0 + w - 1] = 255          # a maximal gradient in the ROI's last column ...
    if pad:
        parent[y0:y0 + h, x0 + w] = 0            # ... against the parent's pixel beside it, which is not part of the frame
    roi = np.ascontiguousarray(parent[y0:y0 + h, x0:x0 + w])
    fin, fout = tmp_path / "parent.raw", tmp_path / "out.raw"
    parent.tofile(fin)
    r = subprocess.run([BIN, str(w), str(h), str(channels), str(fin), "5", str(fout), str(pw * channels), str(x0), str(y0)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    got = np.fromfile(fout, np.uint8).reshape(h, w)
    want = oracle.canny_r(roi, 10, 40)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} pixels differ, first (row, col) {bad[:5].tolist()}"
