"""CPU-only checks of the native stage 2 (aiod_amd.stage2, neural_filter.py, run_pipeline --native_stage2): padder geometry, the
strict state_dict loader against the reference's real key lists (tests/golden/stage2.npz), the CLI's --help and the pipeline's
command list."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stage2.npz")


@pytest.fixture(scope="module")
def g2():
    return dict(np.load(GOLDEN))


def _shapes(table):
    return [tuple(int(v) for v in r if v >= 0) for r in table]


@pytest.mark.parametrize("h,w", [(40, 70), (384, 640), (1080, 1920), (1088, 1920), (32, 33), (1, 1), (31, 63)])
def test_padder_geometry(h, w):
    from aiod_amd.stage2 import padded_size
    Hp, Wp, left = padded_size(h, w)
    x = torch.zeros(1, 1, h, w)
    pw = (((w // 32) + 1) * 32 - w) % 32
    ph = (((h // 32) + 1) * 32 - h) % 32
    y = F.pad(x, [pw // 2, pw - pw // 2, 0, ph], mode="replicate")      # InputPadder mode 'other' (src/models/utils.py:600-612)
    assert (Hp, Wp) == tuple(y.shape[-2:]) and Hp % 32 == 0 and Wp % 32 == 0 and left == pw // 2
    assert padded_size(40, 70) == (64, 96, 13) and padded_size(1080, 1920) == (1088, 1920, 0)


def test_loader_keys_are_the_reference_keys(g2):
    """The loader's key lists are the reference modules' state_dict keys (recorded in the fixture), with exactly the InstanceNorm
    buffers of the TransformNet dropped."""
    from aiod_amd.stage2 import filter_keys, local_keys, NORM_BUFFER
    fk = [(str(k), s) for k, s in zip(g2["filter_keys"], _shapes(g2["filter_shapes"]))]
    lk = [(str(k), s) for k, s in zip(g2["local_keys"], _shapes(g2["local_shapes"]))]
    assert fk == filter_keys()
    dropped = [k for k, _ in lk if NORM_BUFFER.match(k)]
    assert len(dropped) == 3 * 17 and all(".norm_layer." in k for k in dropped)      # 17 normed layers: conv1a..conv3, 10 residual convs, deconv1/2
    assert [(k, s) for k, s in lk if not NORM_BUFFER.match(k)] == local_keys()


def _synthetic(g2, net):
    keys = g2["filter_keys"] if net == 0 else g2["local_keys"]
    shapes = _shapes(g2["filter_shapes"] if net == 0 else g2["local_shapes"])
    return {str(k): torch.zeros(s) for k, s in zip(keys, shapes)}


def test_flatten_is_strict_and_names_the_key(g2):
    from aiod_amd.stage2 import flatten_state_dict, StateDictError, NET_FILTER, NET_LOCAL
    fsd, lsd = _synthetic(g2, 0), _synthetic(g2, 1)
    assert flatten_state_dict(fsd, NET_FILTER).size == sum(v.numel() for v in fsd.values())
    n_norm = sum(v.numel() for k, v in lsd.items() if ".norm_layer." in k)
    assert flatten_state_dict(lsd, NET_LOCAL).size == sum(v.numel() for v in lsd.values()) - n_norm
    bad = dict(fsd); del bad["decoder2.dec2conv1.weight"]
    with pytest.raises(StateDictError, match="missing key 'decoder2.dec2conv1.weight'"):
        flatten_state_dict(bad, NET_FILTER)
    bad = dict(lsd); bad["deconv3.norm_layer.weight"] = torch.zeros(3)
    with pytest.raises(StateDictError, match="unexpected key 'deconv3.norm_layer.weight'"):
        flatten_state_dict(bad, NET_LOCAL)
    bad = dict(fsd); bad["encoder1.norm_layer.running_mean"] = torch.zeros(32)      # norm buffers are ignored on the TransformNet only
    with pytest.raises(StateDictError, match="unexpected key"):
        flatten_state_dict(bad, NET_FILTER)
    bad = dict(lsd); bad["convlstm.Gates.weight"] = torch.zeros(512, 128, 3, 3)
    with pytest.raises(StateDictError, match="'convlstm.Gates.weight' has shape"):
        flatten_state_dict(bad, NET_LOCAL)


def test_flatten_order_and_layout(g2):
    """state_dict order, OIHW row-major, biases after their weights."""
    from aiod_amd.stage2 import flatten_state_dict, local_keys, NET_LOCAL
    lsd = _synthetic(g2, 1)
    off, expect = 0, {}
    for k, s in local_keys():
        n = int(np.prod(s))
        lsd[k] = torch.arange(n, dtype=torch.float32).reshape(s) + off
        expect[k] = off
        off += n
    flat = flatten_state_dict(lsd, NET_LOCAL)
    assert np.array_equal(flat, np.arange(off, dtype=np.float32))


def test_neural_filter_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "all-in-one-deflicker_amd", "neural_filter.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-500:]
    for flag in ("--ckpt_filter", "--ckpt_local", "--fps", "--video_name", "--gpu"):
        assert flag in r.stdout


def test_run_pipeline_native_stage2():
    import importlib.util
    spec = importlib.util.spec_from_file_location("af_run_pipeline", os.path.join(ROOT, "all-in-one-deflicker_amd", "run_pipeline.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    base = dict(video_name="data/test/clip.mp4", video_frame_folder=None, fps=10, gpu=2, class_name=None)
    off = [c for _, c in R.build_commands(argparse.Namespace(**base))]
    assert off[-1] == "python src/neural_filter_and_refinement.py --video_name clip --fps 10"
    off2 = [c for _, c in R.build_commands(argparse.Namespace(native_stage2=False, **base))]
    assert off2 == off
    on = [c for _, c in R.build_commands(argparse.Namespace(native_stage2=True, ckpt_filter="f.pth", ckpt_local="l.pth", **base))]
    assert on[:-1] == off[:-1]
    assert on[-1].endswith("neural_filter.py --video_name clip --fps 10 --gpu 2 --ckpt_filter f.pth --ckpt_local l.pth")
    assert on[-1].startswith(sys.executable or "python")
    # parsed from the command line: off by default
    import unittest.mock as um
    with um.patch.object(R.os, "system", return_value=0) as sysm, um.patch.object(R.os, "makedirs"):
        R.main(["--video_name", "data/test/clip.mp4", "--native_stage2"])
        assert "neural_filter.py --video_name clip" in sysm.call_args_list[-1][0][0]
        R.main(["--video_name", "data/test/clip.mp4"])
        assert "src/neural_filter_and_refinement.py" in sysm.call_args_list[-1][0][0]


def test_fixture_is_small_and_sane(g2):
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert g2["content"].shape == (4, 40, 70, 3) and g2["pred64_hi"].shape == (4, 64, 96, 3)
    rms = dict(zip([str(k) for k in g2["act_names"]], g2["act_rms"]))
    assert all(0.1 < v < 10 for v in rms.values()), rms        # no layer collapsed or exploded
    y = (g2["final64_hi"][1:].astype(np.float64) - g2["pred64_hi"][1:])
    assert 0.01 < np.sqrt((y ** 2).mean()) and np.abs(y).max() < 0.9      # the refinement carries signal; its tanh is not saturated
