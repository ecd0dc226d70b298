"""Host-side checks of what the phases of Deflicker.run must keep as they were (no GPU): the order of the keys of the result, of its laps
and of deflicker.json on every route (the literal lists below were printed by the same calls before `run` was split into phases), that
a run leaves nothing of itself on the Deflicker object, and that a failed run leaves nothing for the next one."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_deflicker_host as TD  # noqa: E402      (each route's own host test defines the stub engines it runs on)
import test_deflicker_seg_host as SH  # noqa: E402
import test_fidelity_host as FH  # noqa: E402
import test_guided_transfer_host as GT  # noqa: E402
import test_maskprop_host as MP  # noqa: E402
import test_render_at_host as RA  # noqa: E402
import test_shots_host as ST  # noqa: E402

HEAD = ["windows", "seam_pairs", "psnr", "arithmetic", "seed", "two_layer", "style_size", "mask_keys", "mask_thresh", "psnr_full", "flow_size",
        "max_long_edge", "flow_precision", "filter_precision", "shots", "cut_pairs", "cuts", "cut_scores"]
MASKS_ONLY = ["masks", "mask_keys", "mask_thresh", "shots", "cut_pairs", "cuts", "cut_scores", "two_layer", "flow_size", "max_long_edge", "flow_precision"]
LAPS = ["decode + flow", "stage 1", "stage 2", "total"]


def _deflicker(E, **kw):
    import aiod_amd
    return aiod_amd.Deflicker(None, None, None, config=TD.SMALL, down=4, seed=7, engines=E, **kw)


def _wide(n):
    return TD._frames(n, 16, 40)


def _reference(n):
    return [f + 50 for f in _wide(n)]


ROUTES = {
    "default": (lambda: _deflicker(TD._StubEngines()).run(TD._frames(9), keep=("final", "stage1", "renders")),
                HEAD + ["final", "stage1", "renders", "seconds"], LAPS),
    "masks": (lambda: SH._deflicker(SH._SegEngines()).run(SH._frames(9), masks=SH._masks(9)),
              HEAD + ["final", "seconds"], LAPS),
    "mask_keys": (lambda: SH._deflicker(MP._KeyEngines()).run(SH._frames(9), mask_keys=MP._keys(0, 8), keep=("final", "masks")),
                  HEAD + ["final", "masks", "seconds"], ["decode + flow", "masks", "stage 1", "stage 2", "total"]),
    "masks_only": (lambda: SH._deflicker(MP._KeyEngines()).run(SH._frames(4), mask_keys=MP._keys(0), masks_only=True),
                   MASKS_ONLY + ["seconds"], ["decode + flow", "masks", "total"]),
    "masks_only, flows kept": (lambda: SH._deflicker(MP._KeyEngines()).run(SH._frames(4), mask_keys=MP._keys(0), masks_only=True, keep=("final", "flows", "masks")),
                               MASKS_ONLY + ["flows", "seconds"], ["decode + flow", "masks", "total"]),
    "cuts": (lambda: _deflicker(ST._StubEngines(), cuts=[5]).run(ST._frames(9), keep=("final", "flows")),
             HEAD + ["final", "flows", "seconds"], LAPS),
    "cuts auto": (lambda: _deflicker(ST._AutoEngines(5), cuts="auto", min_shot_frames=4).run(ST._frames(9)),
                  HEAD + ["final", "seconds"], ["decode + cuts", "flow", "stage 1", "stage 2", "total"]),
    "proxy": (lambda: _deflicker(GT._Engines(), proxy_long_edge=20).run(_wide(4), keep=("final", "stage1")),
              HEAD + ["proxy", "final", "stage1", "seconds"], ["proxy", "decode + flow", "stage 1", "stage 2", "transfer", "total"]),
    "fidelity": (lambda: _deflicker(FH._Engines()).run(_wide(4), fidelity=True, reference=_reference(4), warp_error=True),
                 HEAD + ["warp_error", "fidelity", "final", "seconds"], ["decode + flow", "stage 1", "stage 2", "warp error", "fidelity", "total"]),
    "every route at once": (lambda: _deflicker(FH._Engines(), proxy_long_edge=20).run(_wide(4), fidelity=True, reference=_reference(4), warp_error=True,
                                                                                     keep=("final", "stage1", "filtered", "flows", "renders")),
                            HEAD + ["proxy", "warp_error", "fidelity", "final", "stage1", "filtered", "flows", "renders", "seconds"],
                            ["proxy", "decode + flow", "stage 1", "stage 2", "transfer", "warp error", "fidelity", "total"]),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_result_keys_and_laps_in_order(route):
    run, keys, laps = ROUTES[route]
    res = run()
    assert list(res) == keys
    assert list(res["seconds"]) == laps


RECORD_HEAD = ["windows", "seam_pairs", "psnr", "seconds", "arithmetic", "seed", "two_layer", "flow_size", "max_long_edge", "style_size", "psnr_full",
               "flow_precision", "filter_precision", "shots", "cut_pairs", "cuts", "cut_scores", "mask_keys", "mask_thresh"]
RECORD_TAIL = ["cut_threshold", "cut_margin", "cut_radius", "min_shot_frames", "masks_dir", "mask_keys_dir", "masks_only", "frames", "window_overlap",
               "video", "video_out", "fps", "yuv_layout", "yuv_matrix", "yuv_range"]
RECORDS = {
    "default": (TD._StubEngines, [], RECORD_HEAD + RECORD_TAIL, LAPS),
    "masks_only": (MP._KeyEngines, ["--mask_keys_dir", "KEYS", "--masks_only"],
                   ["seconds", "two_layer", "flow_size", "max_long_edge", "flow_precision", "shots", "cut_pairs", "cuts", "cut_scores", "mask_keys",
                    "mask_thresh"] + RECORD_TAIL, ["decode + flow", "masks", "total"]),
    "fidelity": (FH._Engines, ["--fidelity", "--reference_dir", "CLEAN"], RECORD_HEAD + RECORD_TAIL + ["fidelity", "reference_dir"],
                 ["decode + flow", "stage 1", "stage 2", "fidelity", "total"]),
    "proxy, warp error, fidelity": (FH._Engines, ["--fidelity", "--warp_error", "--proxy_long_edge", "20"],
                                    RECORD_HEAD + ["proxy"] + RECORD_TAIL + ["warp_error", "fidelity", "reference_dir"],
                                    ["proxy", "decode + flow", "stage 1", "stage 2", "transfer", "warp error", "fidelity", "total"]),
}


@pytest.mark.parametrize("route", list(RECORDS))
def test_record_keys_in_order(route, tmp_path):
    from PIL import Image
    from aiod_amd import deflicker
    engines, extra, keys, laps = RECORDS[route]
    clip, clean, key_dir = tmp_path / "clip", tmp_path / "clean", tmp_path / "keys"
    FH._write_seq(clip, 3, 16, 40)
    FH._write_seq(clean, 3, 16, 40, 50)
    key_dir.mkdir()
    Image.fromarray(np.full((5, 7), 101, np.uint8)).save(str(key_dir / "00001.png"))
    (tmp_path / "cfg.json").write_text(json.dumps(SH.SMALL))
    extra = [{"KEYS": str(key_dir), "CLEAN": str(clean)}.get(a, a) for a in extra]
    argv = ["--frames_dir", str(clip), "--out", str(tmp_path / "out"), "--config", str(tmp_path / "cfg.json"), "--seed", "1"] + extra
    assert deflicker.main(argv, engines=engines()) == 0
    rec = json.loads((tmp_path / "out" / "deflicker.json").read_text())
    assert list(rec) == keys
    assert list(rec["seconds"]) == laps


def _same(a, b):
    """Deep equality of two results or engine logs: arrays by value, containers item by item."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_a_run_leaves_nothing_of_itself_on_the_object():
    E = TD._StubEngines()
    d = _deflicker(E)
    before = dict(vars(d))
    d.run(TD._frames(9, 8, 12), keep=("final", "stage1"))
    first = len(E.log)
    res = d.run(TD._frames(7, 16, 20), keep=("final", "stage1"))
    assert vars(d).keys() == before.keys()
    assert all(vars(d)[k] is before[k] for k in before)
    fresh_E = TD._StubEngines()
    fresh = _deflicker(fresh_E).run(TD._frames(7, 16, 20), keep=("final", "stage1"))
    assert res["stage1"].shape == (7, 4, 5, 3) and res["flow_size"] == [16, 20]      # the second clip's sizes, not the first's
    res.pop("seconds"), fresh.pop("seconds")
    assert _same(res, fresh)
    assert _same(E.log[first:], fresh_E.log)


def test_a_failed_run_leaves_nothing_for_the_next():
    E = RA._AtEngines()
    d = _deflicker(E, style_size="full")
    assert len(d.run(TD._frames(9))["psnr_full"]) == 2
    bad = TD._frames(4)
    bad[2] = np.zeros((8, 13, 3), np.uint8)
    with pytest.raises(ValueError, match="frame 2 is 13x8, the first frame 12x8"):
        d.run(bad)
    res = d.run(TD._frames(3, 16, 20), keep=("final", "stage1"))
    assert res["windows"] == [(0, 3)] and len(res["psnr_full"]) == 1      # this run's one window only
    assert res["psnr_full"] == pytest.approx([10 * np.log10(1 / 0.01)])
    assert res["stage1"].shape == (3, 16, 20, 3) and [e for e in E.log if e[0] == "render_at"][-1][2:4] == (16, 20)
