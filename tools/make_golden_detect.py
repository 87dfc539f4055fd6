"""Writes tests/golden/detect.npz: what the reference's own SCRFD.detect returns for the scenes of tests/detect_ref.py (GOLDEN_SCENES).

For use in the build container only, like make_golden_tail.py: it needs the reference checkout, which a clean clone of this repository does
not have.  Usage:  python tools/make_golden_detect.py <reference root>

The reference's module imports cv2 and onnxruntime at use; neither is needed for the lines to be pinned.  The tool cuts distance2bbox,
distance2kps and class SCRFD out of src/utils/dependencies/insightface/model_zoo/scrfd.py with ast and executes just those in a namespace of
its own, builds an instance without __init__, sets by hand the attributes _init_vars would, and gives it
  * a session stub whose run() returns the scene's recorded network outputs, and
  * a cv2 stub whose resize / dnn.blobFromImage are the restatements of tests/detect_ref.py (they only produce the blob the stub session
    ignores: the two cv2 calls stay PARITY UNPINNED).
detect()'s det and kpss are recorded per scene: threshold, decode, order, NMS and the max_num pick are then pinned to the reference's own
code.  Arrays only; nothing of the reference's text is written anywhere."""
import ast
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import detect_ref as DR      # noqa: E402


def load_scrfd(ref_root):
    path = os.path.join(ref_root, "src", "utils", "dependencies", "insightface", "model_zoo", "scrfd.py")
    tree = ast.parse(open(path).read())
    want = {"distance2bbox", "distance2kps", "SCRFD"}
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in want]
    assert {n.name for n in body} == want
    cv2 = types.SimpleNamespace(
        resize=lambda img, size: DR.resize_linear_cv(img, size[1], size[0]),
        dnn=types.SimpleNamespace(blobFromImage=lambda img, scale, size, mean, swapRB: DR.letterbox_blob(img[None], (img.shape[1], img.shape[0]), swapRB)))
    ns = {"np": np, "cv2": cv2}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns["SCRFD"]


class Session:
    def __init__(self, outs):
        self.outs = outs

    def run(self, names, feed):
        return [np.array(o) for o in self.outs]


def detector(SCRFD, outs, n_levels, use_kps):
    d = SCRFD.__new__(SCRFD)
    strides, na = DR.LAYOUTS[n_levels]
    d.session, d.center_cache, d.nms_thresh, d.det_thresh = Session(outs), {}, 0.4, 0.5
    d.input_size, d.batched, d.input_name, d.output_names = None, False, "input", [str(i) for i in range(len(outs))]
    d.input_mean, d.input_std = 127.5, 128.0
    d.use_kps, d._anchor_ratio, d._num_anchors, d.fmc, d._feat_stride_fpn = use_kps, 1.0, na, n_levels, list(strides)
    return d


def main(ref_root):
    SCRFD = load_scrfd(ref_root)
    out = {}
    for name, (det_size, frame_hw, levels, faces, seed, use_kps, max_num, metric) in DR.GOLDEN_SCENES.items():
        outs = DR.synth_outputs(det_size, levels, faces, seed, use_kps=use_kps)
        img = DR.frames_u8(1, frame_hw[0], frame_hw[1], seed)[0]
        det, kpss = detector(SCRFD, outs, levels, use_kps).detect(img, input_size=det_size, max_num=max_num, metric=metric)
        assert det.dtype == np.float32 and (kpss is None) == (not use_kps)
        out[f"{name}/det"] = det
        if use_kps:
            out[f"{name}/kps"] = kpss.astype(np.float32, copy=False)
            assert kpss.dtype == np.float32
        print(name, det.shape)
    path = os.path.join(ROOT, "tests", "golden", "detect.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
