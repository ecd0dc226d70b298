"""Host side of the warping-error report (all-in-one-deflicker_amd/warp_error.py): JSON layouts, sequence discovery, flow-file
pairing, the missing-flow error and the geometry option.  No GPU."""
import json

import numpy as np
import pytest


def _touch_frames(folder, n, ext="png"):
    folder.mkdir(parents=True, exist_ok=True)
    for i in range(n):
        (folder / ("%05d.%s" % (i, ext))).write_bytes(b"")


def test_geometry_parsing():
    from aiod_amd import warp_error as W
    assert W.parse_geometry("exact") is True and W.parse_geometry("reference") is False
    for bad in ("Exact", "align", "", None):
        with pytest.raises(ValueError):
            W.parse_geometry(bad)
    assert W.parse_args(["--vid_name", "v"]).geometry == "exact"
    assert W.parse_args(["--vid_name", "v", "--geometry", "reference"]).geometry == "reference"
    with pytest.raises(SystemExit):
        W.parse_args(["--vid_name", "v", "--geometry", "other"])
    from aiod_amd import stage1  # noqa: F401  (the stage-1 CLIs take --warp_error / --warp_error_geometry)


def test_sequence_discovery(tmp_path):
    from aiod_amd import warp_error as W
    root, res = tmp_path / "data", tmp_path / "results"
    _touch_frames(root / "v", 4, "jpg")
    _touch_frames(res / "v" / "stage_1" / "output", 4)
    _touch_frames(res / "v" / "final" / "output", 1)               # one frame: no pair, not listed
    (res / "v" / "neural_filter").mkdir(parents=True)               # no output folder
    seqs = W.discover_sequences(root, res, "v")
    assert [s[0] for s in seqs] == ["input", "stage_1"]
    assert [p.name for p in seqs[0][2]] == ["%05d.jpg" % i for i in range(4)]
    _touch_frames(res / "v" / "final" / "output", 3)
    _touch_frames(res / "v" / "neural_filter" / "output", 2)
    assert [s[0] for s in W.discover_sequences(root, res, "v")] == ["input", "stage_1", "neural_filter", "final"]
    # mixed extensions sort as the loaders sort them (sorted jpg + png)
    _touch_frames(root / "w", 2, "png")
    (root / "w" / "00001.jpg").write_bytes(b"")
    assert [p.name for p in W.list_frames(root / "w")] == ["00000.png", "00001.jpg", "00001.png"]


def test_flow_pairing_and_missing_file(tmp_path):
    from aiod_amd import warp_error as W
    frames = tmp_path / "v"
    _touch_frames(frames, 3)
    files = W.list_frames(frames)
    fd = tmp_path / "v_flow"
    fd.mkdir()
    for a, b in ((0, 1), (1, 2)):
        for x, y in ((a, b), (b, a)):
            np.save(fd / ("%05d.png_%05d.png.npy" % (x, y)), np.zeros((2, 2, 2), np.float32))
    pairs = W.flow_pairs(files, fd)
    assert [(p.name, q.name) for p, q in pairs] == [("00000.png_00001.png.npy", "00001.png_00000.png.npy"),
                                                    ("00001.png_00002.png.npy", "00002.png_00001.png.npy")]
    (fd / "00002.png_00001.png.npy").unlink()
    with pytest.raises(FileNotFoundError) as e:
        W.flow_pairs(files, fd)
    assert "00002.png_00001.png.npy" in str(e.value) and "preprocess_optical_flow" in str(e.value)


def test_json_layouts():
    from aiod_amd import warp_error as W
    rec = W.eval_record(True, (0.5, np.array([0.25, 0.75])), (0.125, [0.1, 0.15]))
    assert rec == {"geometry": "exact", "align_corners": 1, "input": {"mean": 0.5, "per_pair": [0.25, 0.75]},
                   "reconstruction": {"mean": 0.125, "per_pair": [0.1, 0.15]}}
    assert W.eval_record(False, (0, []), (0, []))["geometry"] == "reference"
    rep = W.report("v", False, [("input", "data/v", 3, (4, 5), 0.2, [0.1, 0.3]), ("final", "results/v/final/output", 3, (2, 3), 0.1, [0.1, 0.1])])
    assert rep["vid_name"] == "v" and rep["geometry"] == "reference" and rep["align_corners"] == 0
    assert list(rep["sequences"]) == ["input", "final"]
    assert rep["sequences"]["input"] == {"path": "data/v", "frames": 3, "height": 4, "width": 5, "mean": 0.2, "per_pair": [0.1, 0.3]}
    json.dumps(rep)          # plain JSON types only
    json.dumps(rec)


def test_read_frame_matches_read_img(tmp_path):
    from PIL import Image
    from aiod_amd import warp_error as W
    im = (np.arange(4 * 5 * 3) * 7 % 256).astype(np.uint8).reshape(4, 5, 3)
    Image.fromarray(im).save(str(tmp_path / "a.png"))
    got = W.read_frame(tmp_path / "a.png")
    assert got.dtype == np.float32 and np.array_equal(got, np.float32(im) / 255.0)
    Image.fromarray(im[:, :, 0]).save(str(tmp_path / "g.png"))
    assert W.read_frame(tmp_path / "g.png").shape == (4, 5, 3)
