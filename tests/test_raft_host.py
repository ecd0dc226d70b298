"""Host-side checks of the native flow precompute (no GPU): the fixture tests/golden/raft.npz against the generator's pure-torch
restatement (and against the live reference modules when a checkout is at AF_REFERENCE or, by default, in `reference/` beside this repository), the strict state_dict loader, the drop-in
CLI's file naming / skip rule / resize refusal with a stubbed flow object, and the --native_flow switches."""
import argparse
import importlib.util
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "raft.npz")
PKG = os.path.join(ROOT, "all-in-one-deflicker_amd")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_raft as G  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def g():
    d = dict(np.load(GOLDEN))
    for k in ("up12", "up21", "lo12", "lo21"):
        d[k] = d[k + "_hi"].astype(np.float64) + d[k + "_lo"].astype(np.float64) / G.LO_SCALE
    sd = {}
    for k, r in zip(d["keys"], d["shapes"]):
        shape = tuple(int(v) for v in r if v >= 0)
        sd[str(k)] = torch.zeros(shape, dtype=torch.int64 if str(k).endswith("num_batches_tracked") else torch.float32)
    G.synthetic_state_dict(sd)
    d["sd"] = sd
    d["err"] = {str(n): e for n, e in zip(d["names"], d["err32"])}
    d["im"] = [G.pad_sintel(G.to_nchw(d["im1"])), G.pad_sintel(G.to_nchw(d["im2"]))]
    return d


def test_fixture_is_small_and_sane(g):
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert g["im1"].shape == (130, 197, 3) and g["up12"].shape == (136, 200, 2) and g["lo12"].shape == (4, 17, 25, 2)
    u1, u2 = G.synthetic_frames()
    np.testing.assert_array_equal(u1, g["im1"]); np.testing.assert_array_equal(u2, g["im2"])
    rms = dict(zip([str(n) for n in g["names"]], g["rms64"]))
    assert 0.5 < rms["lo12_20"] < 5 and 0.5 < rms["lo21_20"] < 5          # flows of a few pixels at full resolution, not noise
    assert rms["net0"] < 0.9 and rms["net"] < 0.95                        # the hidden state is not saturated
    assert (g["err32"] > 0).all()


def test_key_list_matches_the_reference(g):
    from aiod_amd.raft import raft_keys
    assert [k for k, _ in raft_keys()] == [str(k) for k in g["keys"]]
    assert [s for _, s in raft_keys()] == [tuple(int(v) for v in r if v >= 0) for r in g["shapes"]]


def test_restatement_equals_the_fixture(g):
    """The functional restatement in fp64 reproduces the stored twin (computed by the reference's modules); in fp32 it stays within the
    recorded distance of the reference's fp32 run from the twin, times two (two fp32 evaluations of the same function)."""
    torch.set_num_threads(8)
    sd64 = {k: v.double() for k, v in g["sd"].items()}
    for d, (a, b) in (("12", (0, 1)), ("21", (1, 0))):
        lo, up = G.raft_forward(sd64, g["im"][a].double(), g["im"][b].double(), iters=20)
        assert np.abs(up[0].permute(1, 2, 0).numpy() - g["up" + d]).max() < 1e-8
        assert np.abs(lo[0].permute(1, 2, 0).numpy() - g["lo" + d][3]).max() < 1e-9
    lo, up = G.raft_forward(g["sd"], g["im"][0], g["im"][1], iters=20)
    assert np.abs(up[0].permute(1, 2, 0).double().numpy() - g["up12"]).max() <= 2 * g["err"]["up12"][0]
    ref = os.environ.get("AF_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")      # default: a checkout beside this repository
    if os.path.isfile(os.path.join(ref, "src", "models", "stage_1", "core", "raft.py")):      # the live modules, when a checkout is at hand
        model = G.load_reference(ref).double()
        model.load_state_dict(sd64)
        with G.as_double():
            lo_r, up_r = G.ref_run(model, g["im"][0].double(), g["im"][1].double(), 4)
        lo4, up4 = G.raft_forward(sd64, g["im"][0].double(), g["im"][1].double(), iters=4)
        assert np.abs((lo_r - lo4).numpy()).max() < 1e-9 and np.abs((up_r - up4).numpy()).max() < 1e-8


def test_padding():
    from aiod_amd.raft import padded_size
    assert padded_size(130, 197) == (136, 200, 3, 1)
    assert padded_size(432, 768) == (432, 768, 0, 0)
    assert padded_size(1080, 1920) == (1080, 1920, 0, 0)
    x = torch.arange(5 * 7, dtype=torch.float32).reshape(1, 1, 5, 7)
    y = G.pad_sintel(x)
    assert y.shape == (1, 1, 8, 8) and y[0, 0, 0, 0] == x[0, 0, 0, 0] and y[0, 0, 1, 1] == x[0, 0, 0, 1] and y[0, 0, 7, 7] == x[0, 0, 4, 6]


def test_loader_errors(g):
    from aiod_amd.raft import flatten_state_dict
    from aiod_amd import StateDictError
    sd = g["sd"]
    flat = flatten_state_dict(sd)
    n = sum(int(v.numel()) for k, v in sd.items() if not k.endswith("num_batches_tracked"))
    assert flat.dtype == np.float32 and flat.size == n
    np.testing.assert_array_equal(flatten_state_dict({"module." + k: v for k, v in sd.items()}), flat)      # the published layout
    np.testing.assert_array_equal(flat[:64 * 3 * 49], sd["fnet.conv1.weight"].numpy().ravel())
    bad = dict(sd); bad["fnet.norm1.weight"] = torch.zeros(64)
    with pytest.raises(StateDictError, match="unexpected key 'fnet.norm1.weight'"):
        flatten_state_dict(bad)
    bad = dict(sd); del bad["update_block.gru.convq2.bias"]
    with pytest.raises(StateDictError, match="missing key 'update_block.gru.convq2.bias'"):
        flatten_state_dict(bad)
    bad = dict(sd); bad["update_block.gru.convz1.weight"] = torch.zeros(128, 384, 5, 1)
    with pytest.raises(StateDictError, match="convz1.weight' has shape"):
        flatten_state_dict(bad)
    bad = {"module." + k: v for k, v in sd.items()}; bad["cnet.conv1.bias"] = torch.zeros(64)      # mixed prefixes
    with pytest.raises(StateDictError):
        flatten_state_dict(bad)


class _StubFlow:
    def __init__(self, h, w, capacity):
        self.h, self.w, self.capacity, self.encoded, self.calls, self.slots = h, w, capacity, [], [], {}

    def encode(self, slot, img):
        assert img.dtype == np.uint8 and img.shape == (self.h, self.w, 3)
        self.encoded.append(int(img[0, 0, 0]))
        self.slots[slot] = int(img[0, 0, 0])

    def flow_slots(self, pairs):
        self.calls.append(list(pairs))
        hp, wp = (self.h + 7) // 8 * 8, (self.w + 7) // 8 * 8
        return np.stack([np.full((hp, wp, 2), 10 * self.slots[a] + self.slots[b], np.float64) for a, b in pairs])


@pytest.mark.parametrize("capacity", [1, 2])
def test_cli_naming_and_skip_rule(tmp_path, capacity):
    from PIL import Image
    cli = _load("af_pof", os.path.join(PKG, "preprocess_optical_flow.py"))
    vid = tmp_path / "clip"
    vid.mkdir()
    names = ["00000.png", "00001.png", "00002.jpg", "00003.png"]
    for i, n in enumerate(names):
        Image.fromarray(np.full((20, 30, 3), i, np.uint8)).save(vid / n)
    (vid / "notes.txt").write_text("x")                                    # not matched by *.*g
    flow_dir = tmp_path / "clip_flow"
    flow_dir.mkdir()
    np.save(flow_dir / "00002.jpg_00001.png.npy", np.zeros(1))             # ONE file of pair 1 exists: the reference skips the pair
    stubs = []

    def make(h, w):
        stubs.append(_StubFlow(h, w, capacity))
        return stubs[-1]
    args = cli.parse_args(["--vid-path", str(vid)])
    assert args.max_long_edge == 2000 and args.gpu == 0 and args.model == "pretrained_weights/raft-things.pth"
    assert cli.preprocess(args, make) == 2
    got = sorted(p.name for p in flow_dir.iterdir())
    assert got == ["00000.png_00001.png.npy", "00001.png_00000.png.npy", "00002.jpg_00001.png.npy", "00002.jpg_00003.png.npy", "00003.png_00002.jpg.npy"]
    f = np.load(flow_dir / "00000.png_00001.png.npy")
    assert f.dtype == np.float32 and f.shape == (24, 32, 2) and f[0, 0, 0] == 1.0           # frame 0 -> frame 1
    assert np.load(flow_dir / "00001.png_00000.png.npy")[0, 0, 0] == 10.0
    assert np.load(flow_dir / "00002.jpg_00003.png.npy")[0, 0, 0] == 23.0 and np.load(flow_dir / "00003.png_00002.jpg.npy")[0, 0, 0] == 32.0
    assert len(stubs) == 1 and stubs[0].encoded == [0, 1, 2, 3]                             # every needed frame once
    assert len(stubs[0].calls) == (2 if capacity == 2 else 4)
    assert cli.preprocess(args, make) == 0 and len(stubs) == 1                              # everything exists now: nothing to do


def test_cli_refuses_to_resize(tmp_path):
    from PIL import Image
    cli = _load("af_pof2", os.path.join(PKG, "preprocess_optical_flow.py"))
    vid = tmp_path / "big"
    vid.mkdir()
    for n in ("a.png", "b.png"):
        Image.fromarray(np.zeros((16, 40, 3), np.uint8)).save(vid / n)
    with pytest.raises(SystemExit, match="INTER_AREA"):
        cli.preprocess(cli.parse_args(["--vid-path", str(vid), "--max_long_edge", "39"]), lambda h, w: _StubFlow(h, w, 2))
    assert cli.preprocess(cli.parse_args(["--vid-path", str(vid), "--max_long_edge", "40"]), lambda h, w: _StubFlow(h, w, 2)) == 1


def test_native_flow_child_failure_is_fatal():
    """The native flow child's exit status is checked (a missing checkpoint must stop stage 1 with the child's message, not surface
    later as missing .npy files); the reference's scripts keep the reference's own behaviour (status ignored)."""
    import unittest.mock as um
    from aiod_amd import stage1
    base = dict(vid_path="data/test/clip", gpu=0, device_ordinal=0, class_name="portrait")
    with um.patch("subprocess.call", return_value=3) as call:
        with pytest.raises(SystemExit, match="preprocess_optical_flow.py"):
            stage1._run_reference_preprocessors(argparse.Namespace(native_flow=True, **base), False)
        assert call.call_count == 1
    with um.patch("subprocess.call", return_value=0) as call:
        stage1._run_reference_preprocessors(argparse.Namespace(native_flow=True, **base), False)
        assert call.call_count == 1


def test_native_flow_switches():
    from aiod_amd import stage1
    base = dict(vid_path="data/test/clip", gpu=3, device_ordinal=0, class_name="portrait")
    off = stage1._preprocessor_commands(argparse.Namespace(**base), False)
    assert all("all-in-one-deflicker_amd" not in c for c in off)           # default: only the reference's scripts, when ./src has them
    on = stage1._preprocessor_commands(argparse.Namespace(native_flow=True, **base), False)
    assert len(on) == len([c for c in off if "preprocess_optical_flow" not in c]) + 1
    assert on[0].startswith(sys.executable or "python") and "--vid-path data/test/clip --gpu 0" in on[0]
    assert os.path.join("all-in-one-deflicker_amd", "preprocess_optical_flow.py") in on[0]
    assert stage1._preprocessor_commands(argparse.Namespace(native_flow=True, skip_preprocess=True, **base), True) == []
    R = _load("af_run_pipeline_nf", os.path.join(PKG, "run_pipeline.py"))
    b2 = dict(video_name="data/test/clip.mp4", video_frame_folder=None, fps=10, gpu=2, class_name=None)
    off = [c for _, c in R.build_commands(argparse.Namespace(**b2))]
    on = [c for _, c in R.build_commands(argparse.Namespace(native_flow=True, **b2))]
    assert [c for c in on if c.endswith(" --native_flow")] == [c + " --native_flow" for c in off if "stage1.py" in c] and len(on) == len(off)
    on = [c for _, c in R.build_commands(argparse.Namespace(native_flow=True, **dict(b2, class_name="portrait")))]
    assert any("stage1_seg.py" in c and c.endswith("--native_flow") for c in on)
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(PKG, "stage1.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--native_flow" in r.stdout
